"""GPU: the `_scaled` optimizer entry points through the C ABI, `set_scales` through the modules, DINO's weight-decay exclusion, a
resume with scales, and the entry points' flags.  Yardsticks: torch.optim.AdamW with one param group per segment, and the
restatements of tests/optim_ref.py / oracle.mae_oracle.adamw_step_ called per tensor at lr * lr_scale and weight_decay * wd_scale
(tests/param_scales_ref.py; pinned against torch's param groups in tests/test_param_scales_cpu.py).  Lion by the sign rule of
tests/test_optim_gpu.py."""
import logging
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from oracle import mae_oracle as O
from tests import optim_ref as R
from tests import param_scales_ref as P
from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = R.HP
CLIP = 3.0
LION_CAP = 1e-4
# neighbouring one-unit segments with different scales; the 64 K segment spans many blocks
SIZES = [1024, 1024, 3 * 1024, 64 * 1024, 1024, 8 * 1024, 16 * 1024]
LR_SCALES = [1, 0.5, 0.75 ** 3, 0.25, 1, 0, 2]   # [4] is skipped
WD_SCALES = [1, 0, 1, 3, 1, 1, 0]
ZERO_P, HARD, SKIPPED, LR0, ZERO_G = 2, 3, 4, 5, 6
DIAG = ("weight_norm", "adam_norm", "trust_ratio")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _hu(n, seed, dev):
    return torch.from_numpy(O.hash_uniform(n, seed)).to(dev)


def _segments():
    seg = [0]
    for s in SIZES:
        seg.append(seg[-1] + s)
    return seg


def _inputs(dev, step):
    """A fresh hash per step (signs change between steps), scaled per segment: [0] clipped (norm ~ 18), [1] small, [3] clipped hard,
    [5] small, [6] zero."""
    seg = _segments()
    g = _hu(seg[-1], 5200 + step, dev) * (1.0 + 0.1 * step)
    g[seg[1]:seg[2]] *= 1e-3
    g[seg[HARD]:seg[HARD + 1]] *= 100.0
    g[seg[LR0]:seg[LR0 + 1]] *= 0.01
    g[seg[ZERO_G]:seg[ZERO_G + 1]] = 0.0
    return g


def _params(dev):
    seg = _segments()
    p = _hu(seg[-1], 5100, dev)
    p[seg[ZERO_P]:seg[ZERO_P + 1]] = 0.0
    return p


def _ones(dev):
    return torch.ones(len(SIZES), dtype=torch.float32, device=dev)


class _Flat:
    """One flat problem driven through the C ABI.  `scales` None: the unscaled entry point; else (lr_scale, wd_scale) device tensors,
    either of them None for NULL: the `_scaled` one."""

    def __init__(self, lib, kind, dev, momentum=HP["momentum"], scales=None):
        self.lib, self.kind, self.momentum, self.scales = lib, kind, momentum, scales
        seg = self.seg = _segments()
        self.n, self.total = len(SIZES), seg[-1]
        self.p = _params(dev)
        self.g = torch.zeros_like(self.p)
        self.state = {k: torch.zeros_like(self.p) for k in P.STATE_KEYS[kind]} if not (kind == "SGD" and momentum == 0) else {}
        self.diag = {k: torch.full((self.n,), -7.0, device=dev) for k in DIAG}
        self.seg_t = torch.tensor(seg, dtype=torch.int64, device=dev)
        self.skip = torch.tensor([1 if i == SKIPPED else 0 for i in range(self.n)], dtype=torch.uint8, device=dev)
        self.norms, self.coef = torch.empty(self.n, device=dev), torch.empty(self.n, device=dev)
        self.ws = torch.empty(lib.hct_grad_norms_workspace_bytes(self.total), dtype=torch.uint8, device=dev)
        self.lws = torch.empty(lib.hct_lamb_workspace_bytes(self.total, self.n), dtype=torch.uint8, device=dev)
        self.shadow = torch.zeros(self.total, dtype=torch.bfloat16, device=dev)
        self.steps = 0

    def step(self, g, lr=HP["lr"]):
        lib, n, t, kind = self.lib, self.n, self.total, self.kind
        self.steps += 1
        self.g.copy_(g)
        _lib.check(lib.hct_grad_norms(self.g.data_ptr(), self.seg_t.data_ptr(), n, t, CLIP, 0, self.norms.data_ptr(), self.coef.data_ptr(),
                                      self.ws.data_ptr(), self.ws.numel(), _st()), "norms")
        common = (self.seg_t.data_ptr(), self.coef.data_ptr(), self.skip.data_ptr(), n, t)
        sc = None if self.scales is None else tuple(_lib.ptr(s) for s in self.scales)
        if kind == "AdamW":
            args = (self.p.data_ptr(), self.g.data_ptr(), self.state["exp_avg"].data_ptr(), self.state["exp_avg_sq"].data_ptr(), *common, lr,
                    HP["beta1"], HP["beta2"], P.ADAMW_EPS, HP["weight_decay"], self.steps, self.shadow.data_ptr())
            fn, tail = ("hct_adamw_step", ()) if sc is None else ("hct_adamw_step_scaled", sc)
        elif kind == "Lion":
            args = (self.p.data_ptr(), self.g.data_ptr(), self.state["exp_avg"].data_ptr(), *common, lr, HP["beta1"], HP["beta2"],
                    HP["weight_decay"], self.shadow.data_ptr())
            fn, tail = ("hct_lion_step", ()) if sc is None else ("hct_lion_step_scaled", sc)
        elif kind == "SGD":
            buf = self.state["momentum_buffer"].data_ptr() if self.state else None
            args = (self.p.data_ptr(), self.g.data_ptr(), buf, *common, lr, self.momentum, self.shadow.data_ptr())
            fn, tail = ("hct_sgd_step", ()) if sc is None else ("hct_sgd_step_scaled", sc[:1])
        else:
            d = self.diag
            args = (self.p.data_ptr(), self.g.data_ptr(), self.state["exp_avg"].data_ptr(), self.state["exp_avg_sq"].data_ptr(), *common, lr,
                    HP["beta1"], HP["beta2"], R.LAMB_EPS, HP["weight_decay"], d["weight_norm"].data_ptr(), d["adam_norm"].data_ptr(),
                    d["trust_ratio"].data_ptr(), self.lws.data_ptr(), self.lws.numel(), self.shadow.data_ptr())
            fn, tail = ("hct_lamb_step", ()) if sc is None else ("hct_lamb_step_scaled", sc)
        _lib.check(getattr(lib, fn)(*args, *tail, _st()), fn)

    def everything(self):
        return [self.p, self.g, self.shadow] + list(self.state.values()) + list(self.diag.values())


def _clip_(g):
    c = CLIP / (g.norm(2) + 1e-6)
    if c < 1:
        g.mul_(c)
    return g


class _Restated:
    """tests/param_scales_ref.py on per-segment tensors at lr * LR_SCALES[i], wd * WD_SCALES[i], in `dtype` on the device."""

    def __init__(self, kind, dev, dtype, momentum=HP["momentum"]):
        seg = _segments()
        p = _params(dev).to(dtype)
        self.kind, self.dtype, self.hp = kind, dtype, dict(HP, momentum=momentum)
        self.p = [p[seg[i]:seg[i + 1]].clone() for i in range(len(SIZES))]
        self.state = [P.new_state(kind, q, momentum) for q in self.p]
        self.g, self.out = [None] * len(SIZES), [None] * len(SIZES)
        self.excused = [torch.zeros_like(q, dtype=torch.bool) for q in self.p]
        self.steps = 0

    def step(self, g, lr=HP["lr"]):
        seg = _segments()
        self.steps += 1
        for i in range(len(SIZES)):
            if i == SKIPPED:
                continue
            gi = _clip_(g[seg[i]:seg[i + 1]].to(self.dtype).clone())
            self.g[i] = gi
            m_before = self.state[i]["exp_avg"].clone() if self.kind == "Lion" else None
            self.out[i] = P.apply_scaled_(self.kind, self.p[i], gi, self.state[i], lr, self.hp, self.steps, LR_SCALES[i], WD_SCALES[i])
            if self.kind == "Lion":
                self.excused[i] |= R.lion_excused(self.out[i], m_before, gi, self.hp["beta1"])


class _TorchAdamW:
    """torch.optim.AdamW on the device in fp32, one param group per segment."""

    def __init__(self, dev):
        seg = _segments()
        p = _params(dev)
        self.params = [torch.nn.Parameter(p[seg[i]:seg[i + 1]].clone()) for i in range(len(SIZES))]
        groups = [dict(params=[q], lr=HP["lr"] * LR_SCALES[i], weight_decay=HP["weight_decay"] * WD_SCALES[i]) for i, q in enumerate(self.params)]
        self.opt = torch.optim.AdamW(groups, lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=P.ADAMW_EPS, weight_decay=HP["weight_decay"])
        self.p = [q.data for q in self.params]
        self.g = [None] * len(SIZES)
        self.out = [None] * len(SIZES)

    def step(self, g):
        seg = _segments()
        for i, q in enumerate(self.params):
            q.grad = None if i == SKIPPED else _clip_(g[seg[i]:seg[i + 1]].clone())
            self.g[i] = q.grad
        self.opt.step()

    @property
    def state(self):
        return [{k: self.opt.state[q][k] for k in P.STATE_KEYS["AdamW"]} if q in self.opt.state else None for q in self.params]


def _scale_tensors(dev):
    return (torch.tensor(LR_SCALES, dtype=torch.float32, device=dev), torch.tensor(WD_SCALES, dtype=torch.float32, device=dev))


# ---- 1. the kernels against the yardstick ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,momentum", [("AdamW", 0.9), ("Lion", 0.9), ("SGD", 0.9), ("SGD", 0.0), ("Lamb", 0.9)])
def test_scaled_kernels_vs_yardstick(lib, cuda, kind, momentum):
    """hct_grad_norms (clip deferred) + hct_*_step_scaled, 4 steps: parameters, state, the written-back gradient and Lamb's
    diagnostics < 1e-6 relative per segment per step (the bar of test_kernels_vs_restatement / test_clip_and_adamw_vs_torch); the
    skipped segment bit-equal; the lr_scale = 0 segment keeps its parameter bits while its moments advance; shadow == p.to(bf16)."""
    seg = _segments()
    hip = _Flat(lib, kind, cuda, momentum, scales=_scale_tensors(cuda))
    ref = _TorchAdamW(cuda) if kind == "AdamW" else _Restated(kind, cuda, torch.float32, momentum)
    ref64 = _Restated(kind, cuda, torch.float64, momentum) if kind == "Lion" else None
    p0 = hip.p.clone()
    for step in range(4):
        g = _inputs(cuda, step)
        hip.step(g)
        ref.step(g)
        if ref64 is not None:
            ref64.step(g)
        for i in range(len(SIZES)):
            sl = slice(seg[i], seg[i + 1])
            if i == SKIPPED:
                assert torch.equal(hip.p[sl], p0[sl]) and torch.equal(hip.g[sl], g[sl]) and not hip.shadow[sl].any()
                assert all(not s[sl].any() for s in hip.state.values()) and all(float(d[i]) == -7.0 for d in hip.diag.values())
                continue
            if kind == "Lion":
                keep = ~ref64.excused[i]
                share = 1.0 - float(keep.float().mean())
                print(f"step {step} segment {i}: excused share {share:.2e}, rel {rel_err(hip.p[sl][keep], ref.p[i][keep]):.2e}")
                assert share <= LION_CAP, (step, i, share)
                assert rel_err(hip.p[sl][keep], ref.p[i][keep]) < 1e-6, (step, i)
                # an excused element differs by whole steps of 2 * lr_s at most
                assert float((hip.p[sl] - ref.p[i]).abs().max()) <= 2 * HP["lr"] * LR_SCALES[i] * (step + 1) * (1 + 1e-5) + 1e-6
            else:
                e = rel_err(hip.p[sl], ref.p[i])
                print(f"{kind} step {step} segment {i}: parameter rel {e:.2e}")
                assert e < 1e-6, (step, i, e)
            if i == LR0:
                assert torch.equal(hip.p[sl], p0[sl]), (step, i)  # rate 0: not a bit moves, decay included (it is lr_s * wd_s)
            for k, v in hip.state.items():
                if i == ZERO_G:
                    assert not v[sl].any(), (step, i, k)
                else:
                    assert rel_err(v[sl], ref.state[i][k]) < 1e-6, (step, i, k, rel_err(v[sl], ref.state[i][k]))
                    assert v[sl].any()  # the moments advance, at rate 0 too
            if i == ZERO_G:
                assert not hip.g[sl].any()
            else:
                assert rel_err(hip.g[sl], ref.g[i]) < 1e-6  # clipped gradient written back
            if kind == "Lamb":
                for j, k in enumerate(DIAG):
                    a, b = float(hip.diag[k][i]), float(ref.out[i][j])
                    assert abs(a - b) <= 1e-6 * abs(b), (step, i, k, a, b)
        if kind == "Lamb":
            assert float(hip.diag["weight_norm"][HARD]) == 10.0  # ||p|| of 64 K uniform(-1, 1) values: the clamp
            # zero gradient and wd scale 0: u = 0, trust ratio 1, nothing moves
            assert float(hip.diag["adam_norm"][ZERO_G]) == 0.0 and float(hip.diag["trust_ratio"][ZERO_G]) == 1.0
        if kind in ("SGD", "Lamb"):
            assert torch.equal(hip.p[seg[ZERO_G]:seg[ZERO_G + 1]], p0[seg[ZERO_G]:seg[ZERO_G + 1]])
    assert float(hip.coef[0]) < 1.0 and float(hip.coef[HARD]) < 0.01 and float(hip.coef[1]) == 1.0
    # neighbours with different scales really moved differently
    assert not torch.equal(hip.p[seg[0]:seg[1]], p0[seg[0]:seg[1]]) and not torch.equal(hip.p[seg[1]:seg[2]], p0[seg[1]:seg[2]])
    live = torch.ones(hip.total, dtype=torch.bool, device=cuda)
    live[seg[SKIPPED]:seg[SKIPPED + 1]] = False
    assert torch.equal(hip.shadow[live], hip.p[live].to(torch.bfloat16))


# ---- 2. all ones == unscaled ----------------------------------------------------------------------------------------------------
def _run(lib, cuda, kind, scales, momentum=HP["momentum"], steps=3):
    f = _Flat(lib, kind, cuda, momentum, scales=scales)
    for step in range(steps):
        f.step(_inputs(cuda, step), lr=HP["lr"] * (1.0 + 0.37 * step))  # a rate that is no round number in binary
    torch.cuda.synchronize()
    return f.everything()


@pytest.mark.parametrize("kind,momentum", [("AdamW", 0.9), ("Lion", 0.9), ("SGD", 0.9), ("SGD", 0.0), ("Lamb", 0.9)])
def test_all_ones_scales_equal_the_unscaled_call(lib, cuda, kind, momentum):
    """3 steps from equal inputs through the unscaled entry point, `_scaled` with both arrays all ones and `_scaled` with both NULL:
    every bit of parameters, gradient, state, shadow and diagnostics equal.  Then one slot NULL against all ones in that slot."""
    plain = _run(lib, cuda, kind, None, momentum)
    ones = _run(lib, cuda, kind, (_ones(cuda), _ones(cuda)), momentum)
    null = _run(lib, cuda, kind, (None, None), momentum)
    for a, b, c in zip(plain, ones, null):
        assert torch.equal(a, b) and torch.equal(a, c)
    lr_s, wd_s = _scale_tensors(cuda)
    for a, b in zip(_run(lib, cuda, kind, (None, wd_s), momentum), _run(lib, cuda, kind, (_ones(cuda), wd_s), momentum)):
        assert torch.equal(a, b)
    for a, b in zip(_run(lib, cuda, kind, (lr_s, None), momentum), _run(lib, cuda, kind, (lr_s, _ones(cuda)), momentum)):
        assert torch.equal(a, b)
    assert not all(torch.equal(a, b) for a, b in zip(plain, _run(lib, cuda, kind, (lr_s, None), momentum)))  # the scales do something


# ---- 3. reproducibility ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
def test_scaled_kernels_are_bit_reproducible(lib, cuda, kind):
    runs = [[t.clone() for t in _run(lib, cuda, kind, _scale_tensors(cuda))] for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 4. through the modules -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("case", ["plain", "lora"])
def test_finetune_steps_with_scales_vs_restatement(lib, cuda, kind, case):
    """test_finetune_steps_vs_restatement's two steps (B = 8, total-norm clip 1.0, head at 100 x lr) with layer decay 0.5 and the
    no-decay set on the backbone and the no-decay set on the head; `set_scales` is called BEFORE .to(device).  Trainable tensors
    match the restatement fed the HIP path's own gradients at lr * lr_scale, wd * wd_scale (1e-6 x steps; Lion by the sign rule,
    cap over backbone + head), frozen ones keep their bits, the shadow is the rounded parameter.  Then the backbone is re-homed
    (to the CPU and back) and a third step still matches: the uploaded scales follow the buffer."""
    from headct_foundation_amd import LinearClassifier, cross_entropy, layer_decay_scales, no_decay_scales
    from headct_foundation_amd.misc import set_requires_grad_false
    from headct_foundation_amd.optim import clip_grad_norm_, make_optimizer
    torch.manual_seed(4)
    lora = case == "lora"
    vit = P.tiny_vit(lora=lora, compute_dtype="bf16")
    sd = vit.state_dict()
    for n in sd:
        if n in ("cls_token", "register_tokens") or "lora" in n:
            sd[n] = torch.randn(sd[n].shape) * (0.5 if "token" in n else 0.05)
    vit.load_state_dict(sd, strict=True)
    cls = LinearClassifier(48, 2, feature_grad=True)
    lr = {"AdamW": 1e-3, "Lion": 1e-4, "SGD": 1e-3, "Lamb": 1e-3}[kind]
    hp = dict(weight_decay=0.04, beta1=0.9, beta2=0.95, momentum=0.9)
    opts = [make_optimizer(kind, m, r, betas=(0.9, 0.95), weight_decay=0.04, momentum=0.9) for m, r in ((vit, lr), (cls, 100 * lr))]
    opts[0].set_scales(layer_decay_scales(vit, 0.5), no_decay_scales(vit))
    opts[1].set_scales(None, no_decay_scales(cls))
    vit, cls = vit.to(cuda).train(), cls.to(cuda).train()
    if lora:
        set_requires_grad_false(vit, lora=True)
    mods = [(vit, opts[0], lr), (cls, opts[1], 100 * lr)]
    scales = [o.scales() for o in opts]
    assert scales[0]["cls_token"] == (0.125, 0.0) and scales[0]["blocks.1.attn.qkv.weight"] == (0.5, 1.0) and scales[0]["norm.weight"] == (0.5, 0.0)
    assert scales[1] == {"linear.weight": (1.0, 1.0), "linear.bias": (1.0, 0.0)}
    x = (torch.rand(8, 3, 24, 24, 24) * torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0]).view(-1, 1, 1, 1, 1)).to(cuda)
    tg = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=cuda)
    start = [{k: v.detach().clone() for k, v in m.named_parameters()} for m, _, _ in mods]
    mine = [{k: v.clone() for k, v in s.items()} for s in start]
    mine64 = [{k: v.double() for k, v in s.items()} for s in start]
    state = [{k: P.new_state(kind, v) for k, v in s.items()} for s in mine]
    state64 = [{k: P.new_state(kind, v) for k, v in s.items()} for s in mine64]
    excused = [{k: torch.zeros_like(v, dtype=torch.bool) for k, v in s.items()} for s in start]
    total = sum(v.numel() for s in start for v in s.values())

    def one_step(step):
        for _, o, _ in mods:
            o.zero_grad()
        cross_entropy(cls(vit(x)[0]), tg).backward()
        for m, _, _ in mods:
            clip_grad_norm_(m, 1.0)
        grads = [{k: v.grad.detach().clone() for k, v in m.named_parameters() if v.grad is not None} for m, _, _ in mods]
        for _, o, _ in mods:
            o.step()
        torch.cuda.synchronize()
        for j, (m, o, lr_j) in enumerate(mods):
            for k, p in m.named_parameters():
                if k not in grads[j]:
                    assert torch.equal(p.detach(), start[j][k]), (case, k)
                    if p in o.state:
                        assert all(not o.state[p][key].any() for key in P.STATE_KEYS[kind])
                    continue
                a, w = scales[j][k]
                P.apply_scaled_(kind, mine[j][k], grads[j][k], state[j][k], lr_j, hp, step + 1, a, w)
                if kind == "Lion":
                    m_before = state64[j][k]["exp_avg"].clone()
                    c64 = P.apply_scaled_(kind, mine64[j][k], grads[j][k].double(), state64[j][k], lr_j, hp, step + 1, a, w)
                    excused[j][k] |= R.lion_excused(c64, m_before, grads[j][k].double(), hp["beta1"])
                    keep = ~excused[j][k]
                    assert torch.equal(p.detach()[keep], mine[j][k][keep]) or rel_err(p.detach()[keep], mine[j][k][keep]) < 1e-6 * (step + 1), (case, k)
                else:
                    assert rel_err(p.detach(), mine[j][k]) < 1e-6 * (step + 1), (case, k, step, rel_err(p.detach(), mine[j][k]))
                for key in P.STATE_KEYS[kind]:
                    ref = state[j][k][key]
                    assert rel_err(o.state[p][key], ref) < 1e-6 * (step + 1) or float(ref.abs().max()) == 0.0, (case, k, key)
        assert torch.equal(vit._flat_bf16, vit._flat.to(torch.bfloat16))

    for step in range(2):
        one_step(step)
    frozen = {k for k, p in vit.named_parameters() if not p.requires_grad}
    assert bool(frozen) == lora
    for name, off, numel, *_ in vit._layout:  # a frozen segment's state keeps its (zero) bits
        if name in frozen:
            assert all(not opts[0]._flat_buffer(key)[off:off + numel].any() for key in P.STATE_KEYS[kind]), name
    for j, (m, _, _) in enumerate(mods):
        assert any(not torch.equal(p.detach(), start[j][k]) for k, p in m.named_parameters() if p.requires_grad)
    # the uploaded scales are in flat_segments() order on the buffer's device, and follow it when it moves
    def uploaded_ok():
        d = opts[0]._scales_dev
        assert d["flat_id"] == vit._flat.data_ptr() and d["lr"].device == vit._flat.device
        assert d["lr"].tolist() == [scales[0][n][0] for n in vit.flat_segments()[0]] and d["wd"].tolist() == [scales[0][n][1] for n in vit.flat_segments()[0]]
    uploaded_ok()
    vit.to("cpu")
    vit.to(cuda)
    one_step(2)
    uploaded_ok()
    n_ex = sum(int(e.sum()) for d in excused for e in d.values())
    print(f"{kind}/{case}: excused {n_ex} of {total} elements, {len(frozen)} frozen tensors")
    assert n_ex <= int(LION_CAP * total)


# ---- 5. DINO: the weight-decay exclusion as a property -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["AdamW", "Lion", "Lamb"])
def test_dino_excluded_tensors_do_not_see_the_weight_decay(lib, cuda, kind):
    """Two copies of the tiny student, wd_scale = no_decay_scales on both, one at weight_decay 0.4 and one at 0: after one iteration
    on the same crops every excluded tensor is bit-equal between the two and every matrix differs."""
    from headct_foundation_amd import no_decay_scales
    from headct_foundation_amd.dino import DINOLoss, DinoOptimizer
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    torch.manual_seed(6)

    def mk():
        b = ViTBackbone(img_size=24, patch_size=12, in_chans=3, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)
        return MultiCropWrapper(b, DINOHead(48, 512, hidden_dim=64, bottleneck_dim=32)).to(cuda)
    a, b, teacher = mk(), mk(), mk()
    b.load_state_dict(a.state_dict())
    teacher.load_state_dict(a.state_dict())
    crops = [torch.rand(2, 3, 24, 24, 24, device=cuda) for _ in range(4)]
    crit = DINOLoss(512, 4, 0.04, 0.04, 30, 200).to(cuda)
    with torch.no_grad():
        t_out = teacher(crops[:2])['dino_output'].float()
    excluded = no_decay_scales(a)
    assert {"backbone.cls_token", "backbone.patch_embedding.position_embeddings", "backbone.norm.weight", "backbone.blocks.0.mlp.linear1.bias",
            "head.mlp.0.bias", "head.last_layer.weight_g"} <= set(excluded)
    losses = []
    for model, wd in ((a, 0.4), (b, 0.0)):
        opt = DinoOptimizer(model, lr=1e-3, betas=(0.9, 0.95), weight_decay=wd, kind=kind).set_scales(wd_scale=excluded)
        opt.zero_grad()
        crit.center.zero_()
        loss = crit(model(crops)['dino_output'].float(), t_out, 0)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        sd = opt.state_dict()
        assert len(sd["param_groups"]) == 1 and sd["param_groups"][0]["params"] == list(range(len(list(model.parameters()))))
        assert sd["param_groups"][0]["weight_decay"] == wd
    torch.cuda.synchronize()
    assert losses[0] == losses[1] and np.isfinite(losses[0])
    start = dict(teacher.named_parameters())
    for (n, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        if n in excluded:
            assert torch.equal(pa, pb), n
        else:
            assert pa.ndim >= 2 and not torch.equal(pa, pb), n
        assert not torch.equal(pb, start[n]) or pb.grad is None or not pb.grad.any(), n  # the copy without decay trained too


# ---- 6. resume ------------------------------------------------------------------------------------------------------------------
def _config(kind, sched, hp):
    from headct_foundation_amd.cfgnode import CfgNode
    c = CfgNode()
    c.MODEL = CfgNode(); c.MODEL.NAME = "mae"
    c.TRAIN = CfgNode()
    c.TRAIN.GRAD_CLIP, c.TRAIN.OPTIMIZER, c.TRAIN.SCHEDULER = hp["grad_clip"], kind, sched
    c.TRAIN.WEIGHT_DECAY, c.TRAIN.BETA1, c.TRAIN.BETA2, c.TRAIN.MOMENTUM = hp["weight_decay"], hp["beta1"], hp["beta2"], hp["momentum"]
    return c


def test_resume_with_scales_reproduces_uninterrupted_run(lib, cuda, tmp_path):
    """test_resume_reproduces_uninterrupted_run's recipe with AdamW / cosine and scales (the no-decay set, lr scale 0.5 on
    decoder_pred.*): the scales are configuration, so the resumed run sets them again; 3 + 3 steps == 6 steps, bit for bit."""
    from headct_foundation_amd import MaskedAutoencoderViT, no_decay_scales
    from headct_foundation_amd.lr_sched import get_lr_scheduler
    from headct_foundation_amd.misc import load_optimizer, save_checkpoint
    from headct_foundation_amd.optim import clip_gradients, get_optimizer
    cfg = O.CONFIGS["micro"]
    hp = dict(R.CURVE_HP, base_lr=R.CURVE_LR["AdamW"], warmup=2, total=10)

    def fresh(scaled=True):
        m = MaskedAutoencoderViT(**cfg.ctor_kwargs(), compute_dtype="fp32")
        m.load_state_dict(O.make_params(cfg, 0))
        m = m.to(cuda)
        ecfg = _config("AdamW", "cosine", hp)
        opt = get_optimizer(ecfg, hp["base_lr"], [m])
        if scaled:
            opt.set_scales({n: 0.5 for n, _ in m.named_parameters() if n.startswith("decoder_pred.")}, no_decay_scales(m))
        return m, opt, get_lr_scheduler(ecfg, opt, hp["warmup"], hp["total"], hp["min_lr"])

    def steps(m, opt, sch, idx):
        out = []
        for i in idx:
            opt.zero_grad()
            loss, _, _ = m(O.make_volume(cfg, 2, i).to(cuda), noise=O.make_noise(cfg, 2, i).to(cuda))
            loss.backward()
            clip_gradients(m, 3.0)
            opt.step(); sch.step()
            out.append(float(loss.detach()))
        return out

    m, opt, sch = fresh()
    ref = steps(m, opt, sch, range(6))
    m1, opt1, sch1 = fresh()
    first = steps(m1, opt1, sch1, range(3))
    save_checkpoint(m1, None, 0, opt1, sch1, filename="c.pt", best_loss=1.0, dir_add=str(tmp_path), logger=logging.getLogger("t"))
    ck = torch.load(tmp_path / "c.pt", map_location="cpu", weights_only=True)
    assert len(ck["optimizer"]["param_groups"]) == 1 and "lr_scale" not in ck["optimizer"]["param_groups"][0]
    m2, opt2, sch2 = fresh()
    m2.load_state_dict(ck["state_dict"])
    load_optimizer(opt2, sch2, ck, logging.getLogger("t"))
    second = steps(m2, opt2, sch2, range(3, 6))
    assert first + second == ref and ref[-1] < ref[0]
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), n
    a, b = opt.state_dict()["state"], opt2.state_dict()["state"]
    for i in a:
        for k in a[i]:
            assert torch.equal(torch.as_tensor(a[i][k]), torch.as_tensor(b[i][k])), (i, k)
    # and the scales mattered: the same six steps without them end elsewhere
    m3, opt3, sch3 = fresh(scaled=False)
    steps(m3, opt3, sch3, range(6))
    assert not torch.equal(dict(m3.named_parameters())["decoder_pred.bias"], dict(m.named_parameters())["decoder_pred.bias"])


# ---- 7. the entry points -----------------------------------------------------------------------------------------------------------
SCALE_LINE = re.compile(r"parameter scales: lr scale \{([^}]*)\}; (\d+) of (\d+) tensors without weight decay")


def _launch(tmp_path, script, args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    run = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port]
    r = subprocess.run(run + [os.path.join(ROOT, script)] + args, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "nan" not in log.lower().replace("nanosecond", "")
    return log


@pytest.mark.parametrize("flags", [True, False])
def test_main_downstream_layer_decay_and_wd_exclusion(cuda, tmp_path, flags):
    """main_downstream.py on the synthetic tiny configuration, 2 epochs: with --layer_decay 0.75 --wd_exclude_1d the log carries the
    backbone's scale line (0.75^3 embeddings, 0.75^2 block 0, 0.75 block 1 and the final norm) and the count of undecayed tensors;
    without the flags there is no such line."""
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")
    opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48",
            "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1", "MODEL.SAVE_NAME", "ft.pt", "PREDS_SAVE_NAME", "run",
            "MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log")]
    args = ["--cfg", str(cfg), "--model_name", "vit", "--classifier", "linear", "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0",
            "--base_lr", "1e-3"] + (["--layer_decay", "0.75", "--wd_exclude_1d"] if flags else []) + ["--opts"] + opts
    log = _launch(tmp_path, "main_downstream.py", args)
    lines = [l for l in log.splitlines() if SCALE_LINE.search(l)]
    if not flags:
        assert not lines
        return
    back = [SCALE_LINE.search(l) for l in lines if "backbone parameter scales" in l]
    head = [SCALE_LINE.search(l) for l in lines if "classifier parameter scales" in l]
    assert len(back) == 1 and len(head) == 1
    got = {float(part.split(" x")[0]): int(part.split(" x")[1]) for part in back[0].group(1).split(", ")}
    want = {0.75 ** 3, 0.75 ** 2, 0.75}
    assert len(got) == 3 and all(any(abs(g - w) <= 1e-6 * w for g in got) for w in want), got
    import main_downstream
    from headct_foundation_amd import no_decay_scales
    argv = sys.argv
    try:
        sys.argv = ["main_downstream.py"] + args
        vit, cls = main_downstream.build_model(main_downstream.parse_option()[1], torch.device("cpu"))
    finally:
        sys.argv = argv
    n_vit = len(list(vit.parameters()))
    assert sum(got.values()) == n_vit and got[min(got)] == sum(1 for n, _ in vit.named_parameters() if not n.startswith(("blocks.", "norm.")))
    assert (int(back[0].group(2)), int(back[0].group(3))) == (len(no_decay_scales(vit)), n_vit) and 0 < len(no_decay_scales(vit)) < n_vit
    assert head[0].group(1) == "1 x2" and (int(head[0].group(2)), int(head[0].group(3))) == (1, 2)


@pytest.mark.parametrize("flags", [True, False])
def test_main_pretrain_dino_wd_exclusion(cuda, tmp_path, flags):
    """main_pretrain_dino.py on dino_tiny_plumbing.yaml with TRAIN.WD_EXCLUDE_1D True completes and logs the scale line; without it
    there is no such line."""
    args = ["--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "2", "--base_lr", "5e-3", "--cfg",
            os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), "--opts", "MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR",
            str(tmp_path / "log"), "OUTPUT", str(tmp_path / "json")] + (["TRAIN.WD_EXCLUDE_1D", "True"] if flags else [])
    log = _launch(tmp_path, "main_pretrain_dino.py", args)
    found = [SCALE_LINE.search(l) for l in log.splitlines() if SCALE_LINE.search(l)]
    if not flags:
        assert not found
        return
    assert len(found) == 1 and found[0].group(1).startswith("1 x")
    assert 0 < int(found[0].group(2)) < int(found[0].group(3))
