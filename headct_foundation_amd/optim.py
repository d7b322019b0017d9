"""Fused per-parameter gradient clip + AdamW / Lion / SGD / Lamb on the flat parameter buffer (HIP).

Reference semantics:
  * clip_gradients  -- src/utils/misc.py:374-383 (PER-TENSOR L2 clip, coef = clip/(norm+1e-6) applied iff < 1)
  * clip_grad_norm_ -- torch.nn.utils.clip_grad_norm_ as engine_downstream.py:107-111 calls it (ONE norm over all gradients)
  * get_optimizer   -- src/utils/optimizers.py:344-360 (torch.optim.AdamW, one param group, weight decay on
                       every parameter, eps 1e-8)
  * Lion / Lamb     -- src/utils/optimizers.py:267-342 / :154-256; SGD -- torch.optim.SGD(lr, momentum) as :347-353 builds it
`HipAdamW` is a torch.optim.Optimizer whose state_dict()/load_state_dict() are interchangeable with
torch.optim.AdamW's (state = {index: {step, exp_avg, exp_avg_sq}}), so reference checkpoints resume; `HipLion`, `HipSGD` and
`HipLamb` are the same for the reference's `Lion`, `torch.optim.SGD` and `Lamb` state dicts.  What the four share beyond their
kernel lives in `_FlatOptimizer`.
"""
from __future__ import annotations

import math
from itertools import chain
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from ._lib import HctError
from .flat import FlatModule
from .mae import MaskedAutoencoderViT  # noqa: F401 (re-exported for callers)


def unwrap(model):
    """Strip DistributedDataParallel-style wrappers (`.module`)."""
    while hasattr(model, "module") and not isinstance(model, FlatModule):
        model = model.module
    return model


class _FlatState:
    """Device-side bookkeeping shared by the clip and the optimizers for one model."""

    def __init__(self, model):
        self.model = model
        self.flat_id = None
        self.refresh()

    def refresh(self):
        m = self.model
        dev = m._flat.device
        names, seg = m.flat_segments()
        self.names = names
        self.nseg = len(names)
        self.total = seg[-1]
        self.seg_off = torch.tensor(seg, dtype=torch.int64, device=dev)
        named = dict(m.named_parameters())
        self.skip = torch.tensor([0 if named[n].requires_grad else 1 for n in names], dtype=torch.uint8, device=dev)
        self.norms = torch.zeros(self.nseg, dtype=torch.float32, device=dev)
        self.coef = torch.ones(self.nseg, dtype=torch.float32, device=dev)
        lib = _lib.load()
        self.ws = torch.empty(max(16, lib.hct_grad_norms_workspace_bytes(self.total)), dtype=torch.uint8, device=dev)
        self.flat_id = m._flat.data_ptr()
        self.coef_pending = False

    def ensure(self):
        if self.flat_id != self.model._flat.data_ptr():
            self.refresh()


def _state_for(model) -> _FlatState:
    st = getattr(model, "_flat_state", None)
    if st is None:
        st = _FlatState(model)
        model._flat_state = st
    st.ensure()
    return st


def clip_gradients(model, clip: float, defer_to_optimizer: Optional[bool] = None):
    """Per-parameter gradient clipping (src/utils/misc.py:374-383) in one pass, without host syncs.

    Returns the per-parameter L2 norms as a DEVICE tensor in `named_parameters()` order of the parameters
    that have a gradient (the reference returns a Python list after ~250 `.item()` syncs; call `.tolist()`
    on the result if you need that).  When the model is driven by one of the fused optimizers (`HipAdamW`, ...) the scaling itself is folded
    into the optimizer kernel (the clipped gradient is still written back to `.grad` there); otherwise the
    gradients are scaled in place right here.
    """
    m = unwrap(model)
    if not isinstance(m, FlatModule):
        raise HctError("clip_gradients (HIP) expects a flat-buffer HIP model (MaskedAutoencoderViT, ViTBackbone, DINOHead)")
    if not m._flat.is_cuda:
        raise HctError("clip_gradients (HIP) needs the model on a GPU; there is no CPU fallback")
    st = _state_for(m)
    lib = _lib.load()
    defer = m._managed_updates if defer_to_optimizer is None else defer_to_optimizer
    _lib.check(lib.hct_grad_norms(m._flat_grad.data_ptr(), st.seg_off.data_ptr(), st.nseg, st.total, float(clip),
                                  0 if defer else 1, st.norms.data_ptr(), st.coef.data_ptr(), st.ws.data_ptr(),
                                  st.ws.numel(), _lib.stream_ptr()), "hct_grad_norms")
    st.coef_pending = bool(defer)
    # norms in named_parameters() order of the parameters that have a gradient; the gather index lives on the device
    # and is rebuilt only when the set changes (building it every call would be a blocking host->device copy, i.e. a
    # full pipeline drain per step)
    key = tuple(p.grad is not None for p in m.parameters())
    if getattr(st, "norm_key", None) != key:
        order = {n: i for i, n in enumerate(st.names)}
        idx = [order[n] for n, p in m.named_parameters() if p.grad is not None]
        st.norm_idx = torch.tensor(idx, device=st.norms.device, dtype=torch.long)
        st.norm_key = key
    return st.norms[st.norm_idx]


def clip_grad_norm_(model, max_norm: float) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) on a flat-buffer HIP model (the reference's downstream clip,
    engine_downstream.py:107-111): ONE L2 norm over all of the model's gradients, every gradient scaled by
    max_norm / (norm + 1e-6) when that is below 1.  Returns the total norm as a 0-d DEVICE tensor (no host sync).  Unlike
    `clip_gradients` (the per-parameter clip of the pre-training loops) the scaling is always applied here, in place."""
    m = unwrap(model)
    if not isinstance(m, FlatModule):
        raise HctError("clip_grad_norm_ (HIP) expects a flat-buffer HIP model (ViTBackbone, the classification heads, DINOHead, ...)")
    if not m._flat.is_cuda:
        raise HctError("clip_grad_norm_ (HIP) needs the model on a GPU; there is no CPU fallback")
    st = _state_for(m)
    lib = _lib.load()
    tn = getattr(st, "tn_norms", None)
    if tn is None or tn.numel() != st.nseg or tn.device != st.norms.device:
        # own norm / coefficient buffers: a per-parameter clip deferred to the optimizer keeps its coefficients
        st.tn_norms = torch.zeros(st.nseg, dtype=torch.float32, device=st.norms.device)
        st.tn_coef = torch.ones(st.nseg, dtype=torch.float32, device=st.norms.device)
    _lib.check(lib.hct_grad_norms(m._flat_grad.data_ptr(), st.seg_off.data_ptr(), st.nseg, st.total, 0.0, 0, st.tn_norms.data_ptr(),
                                  st.tn_coef.data_ptr(), st.ws.data_ptr(), st.ws.numel(), _lib.stream_ptr()), "hct_grad_norms")
    nrm = torch.empty(2, dtype=torch.float32, device=st.norms.device)
    _lib.check(lib.hct_clip_total_norm(m._flat_grad.data_ptr(), st.total, st.tn_norms.data_ptr(), st.nseg, float(max_norm), nrm.data_ptr(),
                                       _lib.stream_ptr()), "hct_clip_total_norm")
    return nrm[0]


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: one `FlatModule`, one flat fp32 buffer per state quantity with per-parameter views in
    `self.state` under the reference's key names (so `state_dict()` has the reference's layout), re-homing of a loaded state dict
    into those buffers, the skip mask for frozen / gradient-less parameters, the pending clip coefficient of `clip_gradients`,
    and the notifications the model needs (`_managed_updates`, `_grad_overwrite`, `mark_weights_updated`).  A subclass names its
    state buffers (`_BUFFERS`) and launches its kernel (`_launch`)."""

    _BUFFERS = ()  # reference key names of the per-element state, one flat buffer each

    def __init__(self, model, defaults):
        m = unwrap(model)
        if not isinstance(m, FlatModule):
            raise HctError(f"{type(self).__name__} expects a flat-buffer HIP model (MaskedAutoencoderViT, ViTBackbone, DINOHead)")
        self._model = m
        params = list(m.parameters())  # registration order == the torch optimizer's over model.parameters()
        super().__init__(params, defaults)
        self._step_count_fused = 0
        self._bufs = None
        self._scales = {"lr": None, "wd": None}  # name -> multiplier, by slot; None = all ones (configuration, not state)
        self._scales_dev = None
        m._managed_updates = True

    # per-parameter multipliers of the rate and of the weight decay (the reference would use torch param groups)
    def _resolve_scales(self, spec, what):
        if spec is None:
            return None
        named = dict(self._model.named_parameters())
        if callable(spec):
            spec = {n: spec(n, p) for n, p in named.items()}
        elif not isinstance(spec, dict):
            raise TypeError(f"{what}: expected None, a dict of parameter name -> float or a callable (name, parameter) -> float")
        out = {}
        for n, v in spec.items():
            if n not in named:
                raise ValueError(f"{what}: {type(self._model).__name__} has no parameter named {n!r}")
            v = float(v)
            if not math.isfinite(v) or v < 0.0:
                raise ValueError(f"{what}[{n!r}] = {v}: a scale must be finite and >= 0")
            if v != 1.0:
                out[n] = v
        return out or None

    def set_scales(self, lr_scale=None, wd_scale=None):
        """Per-parameter multipliers: parameter `name` is updated at lr * lr_scale[name] with weight decay weight_decay *
        wd_scale[name], whatever the schedules write to the param group.  Each argument is None (all ones), a dict from parameter
        name to float (names not given are 1.0) or a callable (name, parameter) -> float.  The values live on the host by name
        and are uploaded in flat_segments() order when the step needs them, again whenever the flat buffer has moved.  They are
        configuration: state_dict() does not carry them, a resumed run sets them again."""
        lr, wd = self._resolve_scales(lr_scale, "lr_scale"), self._resolve_scales(wd_scale, "wd_scale")
        self._scales = {"lr": lr, "wd": wd}
        self._scales_dev = None
        return self

    def scales(self):
        """{name: (lr_scale, wd_scale)} over every parameter, for logging."""
        lr, wd = self._scales["lr"] or {}, self._scales["wd"] or {}
        return {n: (lr.get(n, 1.0), wd.get(n, 1.0)) for n, _ in self._model.named_parameters()}

    def _scale_ptrs(self, m, st):
        """None when no scale is set (the unscaled entry point runs), else the (lr_scale, wd_scale) device pointers, None for a slot
        that is all ones."""
        if self._scales["lr"] is None and self._scales["wd"] is None:
            return None
        d = self._scales_dev
        if d is None or d["flat_id"] != m._flat.data_ptr():
            d = {"flat_id": m._flat.data_ptr()}
            for slot, vals in self._scales.items():
                d[slot] = None if vals is None else torch.tensor([vals.get(n, 1.0) for n in st.names], dtype=torch.float32, device=m._flat.device)
            self._scales_dev = d
        return _lib.ptr(d["lr"]), _lib.ptr(d["wd"])

    def _buffer_keys(self):
        return self._BUFFERS

    def _entry(self, views, seg, prev):
        """state[p] of one parameter: its views into the flat buffers (+ what a subclass adds; `seg` = its segment index, `prev` = the
        entry it had before, e.g. freshly loaded)."""
        return views

    # flat state buffers, exposed per-parameter through self.state for state_dict() compatibility
    def _ensure_state(self):
        m = self._model
        keys = tuple(self._buffer_keys())
        b = self._bufs
        if b is not None and b["device"] == m._flat.device and b["numel"] == m._flat.numel() and b["keys"] == keys:
            return
        old = {id(p): self.state.get(p) for p in m.parameters()}
        self._bufs = {"device": m._flat.device, "numel": m._flat.numel(), "keys": keys, "flat": {k: torch.zeros_like(m._flat) for k in keys}}
        self._alloc_extra(m)
        named = dict(m.named_parameters())
        seg = {n: i for i, n in enumerate(m.flat_segments()[0])}
        for name, off, numel, shape, rg, _ in m._layout:
            p = named[name]
            if not p.requires_grad:
                continue
            prev = old.get(id(p))
            views = {}
            for k in keys:
                views[k] = self._bufs["flat"][k][off:off + numel].view(shape)
                if prev and prev.get(k) is not None:
                    views[k].copy_(prev[k])
            entry = self._entry(views, seg[name], prev)
            if entry:
                self.state[p] = entry
            else:
                self.state.pop(p, None)

    def _alloc_extra(self, m):
        pass

    def _flat_buffer(self, key):
        return self._bufs["flat"][key]

    def _loaded_step(self) -> int:
        steps = [float(s["step"]) for s in self.state.values() if "step" in s]
        return int(max(steps)) if steps else 0

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # re-home the loaded state into the flat buffers
        self._step_count_fused = self._loaded_step()
        self._after_load()
        self._bufs = None
        self._ensure_state()

    def _after_load(self):
        pass

    def zero_grad(self, set_to_none: bool = True):
        super().zero_grad(set_to_none=set_to_none)
        self._model._grad_overwrite = True

    def _launch(self, lib, m, st, grp, coef, scales):
        """One step.  `scales` is None (the unscaled entry point, as before there were scales) or the two device pointers for the
        `_scaled` one."""
        raise NotImplementedError

    def _after_launch(self):
        pass

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        m = self._model
        if not m._flat.is_cuda:
            raise HctError(f"{type(self).__name__}.step needs the model on a GPU; there is no CPU fallback")
        self._ensure_state()
        st = _state_for(m)
        grp = self.param_groups[0]
        self._step_count_fused += 1
        lib = _lib.load()
        coef = st.coef.data_ptr() if st.coef_pending else None
        # parameters that received no gradient this step are skipped like torch does (p.grad is None): the skip mask follows the
        # set of gradient-less parameters and is re-uploaded only when that set changes (e.g. the DINO prototype layer, whose
        # gradients are cancelled during the first epochs)
        named = getattr(m, "_named_cache", None) or dict(m.named_parameters())
        key = tuple((not named[n].requires_grad) or named[n].grad is None for n in st.names)
        if getattr(st, "skip_key", None) != key:
            st.skip = torch.tensor([1 if k else 0 for k in key], dtype=torch.uint8, device=m._flat.device)
            st.skip_key = key
        self._skipped = dict(zip(st.names, key))
        self._launch(lib, m, st, grp, coef, self._scale_ptrs(m, st))
        st.coef_pending = False
        self._after_launch()
        m.mark_weights_updated(plain_bf16_fresh=m._flat_bf16 is not None)
        return loss


class HipAdamW(_FlatOptimizer):
    """torch.optim.AdamW semantics, executed as one fused HIP kernel over the model's flat buffers."""

    _BUFFERS = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(model, defaults)

    # torch.optim.AdamW counts updates per parameter: one with `grad is None` is passed over, and its bias corrections start at 1
    # when it first receives a gradient (the DINO prototype layer after DINO.FREEZE_LAST_LAYER epochs).  `_seg_steps` holds the
    # count of every segment on the host, which knows it from the skip key it forms each step anyway.  While all live segments
    # share one count the launch is hct_adamw_step[_scaled] with that count; once they differ it is hct_adamw_step_counts with
    # the counts in a device array that an in-stream add keeps current (uploaded again only when the skip key changes).
    def _alloc_extra(self, m):
        names = m.flat_segments()[0]
        named = dict(m.named_parameters())
        self._seg_steps = np.zeros(len(names), dtype=np.int64)
        self._seg_trainable = np.array([named[n].requires_grad for n in names], dtype=bool)
        self._seg_entries = [None] * len(names)
        self._live_key = self._live = None
        self._uniform, self._uniform_step, self._first_live, self._all_live = True, 1, -1, False
        self._steps_dev = self._steps_dev_host = self._live_dev = self._steps_dev_key = None
        self._step_tensor = None  # the one CPU scalar every entry shares while all trainable segments have the same count

    def _entry(self, views, seg, prev):
        count = int(float(prev["step"])) if prev and "step" in prev else 0
        self._seg_steps[seg] = count
        self._seg_entries[seg] = entry = {"step": torch.tensor(float(count)), **views}
        return entry

    def _launch(self, lib, m, st, grp, coef, scales):
        key = st.skip_key
        live, steps = self._live, self._seg_steps
        if key != self._live_key:  # whether the live counts agree, and whether every trainable segment is live, can change only here
            self._live_key, self._live = key, ~np.array(key, dtype=bool)
            live = self._live
            steps += live
            now = steps[live]
            self._uniform = bool(now.size == 0 or (now == now[0]).all())
            self._uniform_step = int(now[0]) if now.size else 1
            self._first_live = int(np.argmax(live)) if now.size else -1
            self._all_live = bool(live[self._seg_trainable].all())
        else:
            steps += live
            if self._first_live >= 0:
                self._uniform_step = int(steps[self._first_live])  # every live segment's count, where they agree
        head = (m._flat.data_ptr(), m._flat_grad.data_ptr(), self._flat_buffer("exp_avg").data_ptr(), self._flat_buffer("exp_avg_sq").data_ptr(),
                st.seg_off.data_ptr(), coef, st.skip.data_ptr(), st.nseg, st.total, float(grp["lr"]), float(grp["betas"][0]),
                float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]))
        if self._uniform:
            args = head + (self._uniform_step, _lib.ptr(m._flat_bf16))
            if scales is None:
                _lib.check(lib.hct_adamw_step(*args, _lib.stream_ptr()), "hct_adamw_step")
            else:
                _lib.check(lib.hct_adamw_step_scaled(*args, *scales, _lib.stream_ptr()), "hct_adamw_step_scaled")
            return
        if self._steps_dev is not None and self._steps_dev_key == key and np.array_equal(self._steps_dev_host + live, steps):
            self._steps_dev.add_(self._live_dev)
        else:
            dev = m._flat.device
            self._steps_dev = torch.tensor(steps, dtype=torch.int32, device=dev)
            self._live_dev = torch.tensor(live, dtype=torch.int32, device=dev)
            self._steps_dev_key = key
        self._steps_dev_host = steps.copy()
        _lib.check(lib.hct_adamw_step_counts(*head, self._steps_dev.data_ptr(), _lib.ptr(m._flat_bf16), *(scales or (None, None)),
                                             _lib.stream_ptr()), "hct_adamw_step_counts")

    def _after_launch(self):
        # state[p]["step"]: the parameter's own count.  One shared CPU scalar while every trainable segment has the same count (one
        # fill per step); otherwise one scalar per distinct count, shared by the entries that have it
        if self._step_tensor is not None and self._all_live:  # they agreed, and all moved together
            self._step_tensor.fill_(float(self._uniform_step))
            return
        counts = self._seg_steps[self._seg_trainable]
        if counts.size == 0:
            return
        if (counts == counts[0]).all():
            if self._step_tensor is None:
                self._step_tensor = torch.tensor(0.0)
                for e in self._seg_entries:
                    if e is not None:
                        e["step"] = self._step_tensor
            self._step_tensor.fill_(float(counts[0]))
            return
        self._step_tensor = None
        by_count = {}
        for c, e in zip(self._seg_steps.tolist(), self._seg_entries):
            if e is not None:
                t = by_count.get(c)
                if t is None:
                    t = by_count[c] = torch.tensor(float(c))
                e["step"] = t


class HipLion(_FlatOptimizer):
    """The reference's `Lion` (src/utils/optimizers.py:267-342, `use_triton=False`) as one fused HIP kernel: decoupled weight decay,
    p -= lr * sign(beta1 * m + (1 - beta1) * g), then m <- beta2 * m + (1 - beta2) * g.  State per parameter: `exp_avg`."""

    _BUFFERS = ("exp_avg",)

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.99), weight_decay=0.0):
        assert lr > 0.0 and all(0.0 <= b <= 1.0 for b in betas), f"HipLion needs lr > 0 and betas in [0, 1]: got lr={lr}, betas={betas}"
        super().__init__(model, dict(lr=lr, betas=betas, weight_decay=weight_decay))

    def _launch(self, lib, m, st, grp, coef, scales):
        args = (m._flat.data_ptr(), m._flat_grad.data_ptr(), self._flat_buffer("exp_avg").data_ptr(), st.seg_off.data_ptr(), coef,
                st.skip.data_ptr(), st.nseg, st.total, float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]),
                float(grp["weight_decay"]), _lib.ptr(m._flat_bf16))
        if scales is None:
            _lib.check(lib.hct_lion_step(*args, _lib.stream_ptr()), "hct_lion_step")
        else:
            _lib.check(lib.hct_lion_step_scaled(*args, *scales, _lib.stream_ptr()), "hct_lion_step_scaled")


class HipSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum) as the reference builds it (src/utils/optimizers.py:347-353: no weight decay, dampening 0, no
    Nesterov) as one fused HIP kernel.  State per parameter: `momentum_buffer`; none with momentum 0.  The param group carries
    torch.optim.SGD's keys, and a `weight_decay` written there (DINO's schedule does) is ignored, as the reference's SGD ignores it."""

    def __init__(self, model, lr=1e-3, momentum=0.0):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        super().__init__(model, dict(lr=lr, momentum=momentum, dampening=0, weight_decay=0, nesterov=False, maximize=False, foreach=None,
                                     differentiable=False, fused=None))

    def _buffer_keys(self):
        return ("momentum_buffer",) if self.param_groups[0]["momentum"] != 0 else ()

    def _launch(self, lib, m, st, grp, coef, scales):
        buf = self._flat_buffer("momentum_buffer").data_ptr() if grp["momentum"] != 0 else None
        args = (m._flat.data_ptr(), m._flat_grad.data_ptr(), buf, st.seg_off.data_ptr(), coef, st.skip.data_ptr(), st.nseg, st.total,
                float(grp["lr"]), float(grp["momentum"]), _lib.ptr(m._flat_bf16))
        if scales is None:
            _lib.check(lib.hct_sgd_step(*args, _lib.stream_ptr()), "hct_sgd_step")
        else:
            _lib.check(lib.hct_sgd_step_scaled(*args, scales[0], _lib.stream_ptr()), "hct_sgd_step_scaled")  # a wd_scale is ignored, as the decay is


class HipLamb(_FlatOptimizer):
    """Lamb with the arithmetic of the reference's `lamb_kernel` (src/utils/optimizers.py:154-172, what `JITLamb` runs): moments
    without bias correction, u = m / (sqrt(v) + eps) + wd * p, trust ratio min(||p||, 10) / (||u|| + eps) per tensor (1 where either
    norm is 0).  NOT the class `Lamb` that the reference's `get_optimizer` names: its first moment accumulates the SQUARED gradient
    (:120), which does not descend.  The state dict keeps that class's layout: {step (int), exp_avg, exp_avg_sq,
    weight_norm, adam_norm, trust_ratio}, the last three 0-d views of per-segment device arrays (no host sync)."""

    _BUFFERS = ("exp_avg", "exp_avg_sq")
    _DIAG = ("weight_norm", "adam_norm", "trust_ratio")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0, adam=False):
        if lr < 0.0 or eps < 0.0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"HipLamb needs lr >= 0, eps >= 0 and betas in [0, 1): got lr={lr}, eps={eps}, betas={betas}")
        if adam:
            raise NotImplementedError("HipLamb: adam=True (trust ratio forced to 1) is not on the HIP path")
        self.adam = False
        self._ws = None
        super().__init__(model, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _alloc_extra(self, m):
        nseg = len(m.flat_segments()[0])
        self._diag = {k: torch.zeros(nseg, dtype=torch.float32, device=m._flat.device) for k in self._DIAG}
        self._ws = None

    def _entry(self, views, seg, prev):
        entry = {"step": int(prev["step"]) if prev and "step" in prev else 0, **views}
        for k in self._DIAG:
            entry[k] = self._diag[k][seg]
            if prev and prev.get(k) is not None:  # a tensor, or the int 1 the reference stores for a zero norm
                entry[k].copy_(torch.as_tensor(prev[k], dtype=torch.float32))
        return entry

    def _launch(self, lib, m, st, grp, coef, scales):
        if self._ws is None:
            self._ws = torch.empty(max(16, lib.hct_lamb_workspace_bytes(st.total, st.nseg)), dtype=torch.uint8, device=m._flat.device)
        d = self._diag
        args = (m._flat.data_ptr(), m._flat_grad.data_ptr(), self._flat_buffer("exp_avg").data_ptr(), self._flat_buffer("exp_avg_sq").data_ptr(),
                st.seg_off.data_ptr(), coef, st.skip.data_ptr(), st.nseg, st.total, float(grp["lr"]), float(grp["betas"][0]),
                float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]), d["weight_norm"].data_ptr(), d["adam_norm"].data_ptr(),
                d["trust_ratio"].data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.ptr(m._flat_bf16))
        if scales is None:
            _lib.check(lib.hct_lamb_step(*args, _lib.stream_ptr()), "hct_lamb_step")
        else:
            _lib.check(lib.hct_lamb_step_scaled(*args, *scales, _lib.stream_ptr()), "hct_lamb_step_scaled")

    def _after_launch(self):
        # `step` counts the updates a parameter has received, as the reference's does (it skips p.grad is None): a segment
        # skipped this time keeps its count with the rest of its state
        named = getattr(self._model, "_named_cache", None) or dict(self._model.named_parameters())
        for name, skipped in self._skipped.items():
            if not skipped:
                self.state[named[name]]["step"] += 1


OPTIMIZERS = ("SGD", "AdamW", "Lamb", "Lion")


def make_optimizer(kind, model, lr, betas=(0.9, 0.999), weight_decay=0.0, momentum=0.0, eps=None):
    """One fused optimizer of the given TRAIN.OPTIMIZER kind with the arguments the reference's get_optimizer passes
    (src/utils/optimizers.py:344-379): SGD takes lr and momentum only, the others lr, weight decay and betas.  `eps` (AdamW, Lamb)
    stays at the class default unless given."""
    extra = {} if eps is None else {"eps": eps}
    if kind == "SGD":
        return HipSGD(model, lr=lr, momentum=momentum)
    if kind == "AdamW":
        return HipAdamW(model, lr=lr, weight_decay=weight_decay, betas=betas, **extra)
    if kind == "Lamb":
        return HipLamb(model, lr=lr, weight_decay=weight_decay, betas=betas, **extra)
    if kind == "Lion":
        return HipLion(model, lr=lr, weight_decay=weight_decay, betas=betas)
    raise NotImplementedError("Unknown optimizer: {}".format(kind))


def get_optimizer(config, lr, models):
    """src/utils/optimizers.py:344-379: TRAIN.OPTIMIZER = 'SGD' | 'AdamW' | 'Lamb' | 'Lion' over one flat-buffer model.  With
    TRAIN.WD_EXCLUDE_1D the parameters of `param_scales.no_decay_scales` get a weight-decay scale of 0."""
    if config.TRAIN.OPTIMIZER not in OPTIMIZERS:
        raise NotImplementedError("Unknown optimizer: {}".format(config.TRAIN.OPTIMIZER))
    if len(models) != 1:
        raise HctError("get_optimizer (HIP) expects exactly one model")
    opt = make_optimizer(config.TRAIN.OPTIMIZER, models[0], lr, betas=(config.TRAIN.BETA1, config.TRAIN.BETA2),
                         weight_decay=config.TRAIN.WEIGHT_DECAY, momentum=config.TRAIN.MOMENTUM)
    if getattr(config.TRAIN, "WD_EXCLUDE_1D", False):  # an addition of this build; off = the reference's one group that decays everything
        from .param_scales import no_decay_scales
        opt.set_scales(wd_scale=no_decay_scales(unwrap(models[0])))
    return opt
