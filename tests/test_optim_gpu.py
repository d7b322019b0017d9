"""GPU: the Lion / SGD / Lamb kernels through the C ABI, and the optimizers / schedules in the MAE step, a downstream fine-tuning
step, a DINO iteration and a resume.  Yardsticks: tests/optim_ref.py (the restatement the fixture generator asserted against the
reference's own classes) run in fp32 on the same device, and tests/golden/optimizers.json (the reference's own train_one_epoch).

Lion's sign is discontinuous: an element whose c = beta1*m + (1-beta1)*g cancels to rounding may legitimately step the other way.
Parameters are compared on all elements except those with |c| <= 1e-5 * (beta1*|m| + (1-beta1)*|g|) in the fp64 restatement at any
step so far (optim_ref.lion_excused), and that set may hold at most 1e-4 of the elements (per tensor for the kernel tests, of the
whole model where the tensors are small)."""
import logging
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from headct_foundation_amd import _lib
from oracle import mae_oracle as O
from tests import optim_ref as R
from tests.util import build_hip_model, load_golden, rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = R.HP
CLIP = 3.0
# clipped | clipped, ||p|| > 10 | not clipped | skipped | zero parameter | zero gradient
SIZES = [64 * 1024, 192 * 1024, 128 * 1024, 1024, 8 * 1024, 16 * 1024]
SKIPPED, ZERO_P, ZERO_G = 3, 4, 5
LION_CAP = 1e-4


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
    """uniform(-1, 1) parameters; gradients from a fresh hash per step (signs change between steps), scaled per segment."""
    seg = _segments()
    g = _hu(seg[-1], 4200 + step, dev) * (1.0 + 0.1 * step)
    g[seg[0]:seg[1]] *= 0.05      # norm ~ 7: clipped
    g[seg[1]:seg[2]] *= 100.0     # clipped hard
    g[seg[2]:seg[3]] *= 1e-3      # not clipped
    g[seg[4]:seg[5]] *= 0.01      # not clipped
    g[seg[5]:seg[6]] = 0.0
    return g


def _params(dev):
    seg = _segments()
    p = _hu(seg[-1], 4100, dev)
    p[seg[ZERO_P]:seg[ZERO_P + 1]] = 0.0
    return p


class _Flat:
    """One flat problem driven through the C ABI."""

    def __init__(self, lib, kind, dev, momentum=HP["momentum"]):
        self.lib, self.kind, self.momentum = lib, kind, momentum
        seg = self.seg = _segments()
        self.n, self.total = len(SIZES), seg[-1]
        self.p = _params(dev)
        self.g = torch.zeros_like(self.p)
        self.state = {k: torch.zeros_like(self.p) for k in R.STATE_KEYS[kind]} if not (kind == "SGD" and momentum == 0) else {}
        self.diag = {k: torch.full((self.n,), -7.0, device=dev) for k in ("weight_norm", "adam_norm", "trust_ratio")}
        self.seg_t = torch.tensor(seg, dtype=torch.int64, device=dev)
        self.skip = torch.tensor([1 if i == SKIPPED else 0 for i in range(self.n)], dtype=torch.uint8, device=dev)
        self.norms, self.coef = torch.empty(self.n, device=dev), torch.empty(self.n, device=dev)
        self.ws = torch.empty(lib.hct_grad_norms_workspace_bytes(self.total), dtype=torch.uint8, device=dev)
        self.lws = torch.empty(lib.hct_lamb_workspace_bytes(self.total, self.n), dtype=torch.uint8, device=dev)
        self.shadow = torch.zeros(self.total, dtype=torch.bfloat16, device=dev)

    def step(self, g, lr=HP["lr"]):
        lib, n, t = self.lib, self.n, self.total
        self.g.copy_(g)
        _lib.check(lib.hct_grad_norms(self.g.data_ptr(), self.seg_t.data_ptr(), n, t, CLIP, 0, self.norms.data_ptr(), self.coef.data_ptr(),
                                      self.ws.data_ptr(), self.ws.numel(), _st()), "norms")
        common = (self.seg_t.data_ptr(), self.coef.data_ptr(), self.skip.data_ptr(), n, t)
        if self.kind == "Lion":
            rc = lib.hct_lion_step(self.p.data_ptr(), self.g.data_ptr(), self.state["exp_avg"].data_ptr(), *common, lr, HP["beta1"], HP["beta2"],
                                   HP["weight_decay"], self.shadow.data_ptr(), _st())
        elif self.kind == "SGD":
            buf = self.state["momentum_buffer"].data_ptr() if self.state else None
            rc = lib.hct_sgd_step(self.p.data_ptr(), self.g.data_ptr(), buf, *common, lr, self.momentum, self.shadow.data_ptr(), _st())
        else:
            d = self.diag
            rc = lib.hct_lamb_step(self.p.data_ptr(), self.g.data_ptr(), self.state["exp_avg"].data_ptr(), self.state["exp_avg_sq"].data_ptr(), *common,
                                   lr, HP["beta1"], HP["beta2"], R.LAMB_EPS, HP["weight_decay"], d["weight_norm"].data_ptr(), d["adam_norm"].data_ptr(),
                                   d["trust_ratio"].data_ptr(), self.lws.data_ptr(), self.lws.numel(), self.shadow.data_ptr(), _st())
        _lib.check(rc, self.kind)

    def everything(self):
        return [self.p, self.g, self.shadow] + list(self.state.values()) + list(self.diag.values())


def _clip_(g):
    c = CLIP / (g.norm(2) + 1e-6)
    if c < 1:
        g.mul_(c)
    return g


class _Restated:
    """tests/optim_ref.py on per-segment tensors, in `dtype` on the device."""

    def __init__(self, kind, dev, dtype, momentum=HP["momentum"]):
        seg = _segments()
        p = _params(dev).to(dtype)
        self.kind, self.dtype, self.hp = kind, dtype, dict(HP, momentum=momentum)
        self.p = [p[seg[i]:seg[i + 1]].clone() for i in range(len(SIZES))]
        self.state = [R.new_state(kind, q, momentum) for q in self.p]
        self.g, self.out = [None] * len(SIZES), [None] * len(SIZES)
        self.excused = [torch.zeros_like(q, dtype=torch.bool) for q in self.p]

    def step(self, g, lr=HP["lr"]):
        seg = _segments()
        for i in range(len(SIZES)):
            if i == SKIPPED:
                continue
            gi = _clip_(g[seg[i]:seg[i + 1]].to(self.dtype).clone())
            self.g[i] = gi
            m_before = self.state[i]["exp_avg"].clone() if self.kind == "Lion" else None
            self.out[i] = R.apply_(self.kind, self.p[i], gi, self.state[i], lr, self.hp)
            if self.kind == "Lion":
                self.excused[i] |= R.lion_excused(self.out[i], m_before, gi, self.hp["beta1"])


@pytest.mark.parametrize("kind,momentum", [("Lion", 0.9), ("SGD", 0.9), ("SGD", 0.0), ("Lamb", 0.9)])
def test_kernels_vs_restatement(lib, cuda, kind, momentum):
    """hct_grad_norms + hct_{lion,sgd,lamb}_step against the restatement + the reference's per-tensor clip, shaped like
    test_clip_and_adamw_vs_torch: parameters, state and the written-back gradient < 1e-6 relative per segment, skipped segment
    bit-equal (parameter, state, shadow, diagnostics), shadow == p.to(bfloat16), Lamb's diagnostics < 1e-6; ||p|| > 10, a zero
    parameter and a zero gradient among the segments."""
    seg = _segments()
    hip, ref, ref64 = _Flat(lib, kind, cuda, momentum), _Restated(kind, cuda, torch.float32, momentum), _Restated(kind, cuda, torch.float64, momentum)
    p0 = hip.p.clone()
    assert float(p0[seg[1]:seg[2]].norm()) > 10
    for step in range(4):
        g = _inputs(cuda, step)
        hip.step(g)
        ref.step(g)
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
                # an excused element differs by whole steps of 2*lr at most, never by anything else
                assert float((hip.p[sl] - ref.p[i]).abs().max()) <= 2 * HP["lr"] * (step + 1) * (1 + 1e-5) + 1e-6
            else:
                assert rel_err(hip.p[sl], ref.p[i]) < 1e-6, (step, i, rel_err(hip.p[sl], ref.p[i]))
            for k, v in hip.state.items():
                if i == ZERO_G:
                    assert not v[sl].any(), (step, i, k)
                else:
                    assert rel_err(v[sl], ref.state[i][k]) < 1e-6, (step, i, k)
            assert rel_err(hip.g[sl], ref.g[i]) < 1e-6 or i == ZERO_G  # clipped gradient written back
            if i == ZERO_G:
                assert not hip.g[sl].any()
            if kind == "Lamb":
                for j, k in enumerate(("weight_norm", "adam_norm", "trust_ratio")):
                    a, b = float(hip.diag[k][i]), float(ref.out[i][j])
                    assert abs(a - b) <= 1e-6 * abs(b), (step, i, k, a, b)
        if kind == "Lamb":
            assert float(hip.diag["weight_norm"][1]) == 10.0                                    # the clamp
            if step == 0:
                assert float(hip.diag["weight_norm"][ZERO_P]) == 0.0 and float(hip.diag["trust_ratio"][ZERO_P]) == 1.0
            an, pn = float(hip.diag["adam_norm"][ZERO_G]), float(hip.p[seg[ZERO_G]:seg[ZERO_G + 1]].norm())
            assert abs(an - HP["weight_decay"] * pn) < 1e-3 * an                              # a = wd * ||p|| (p before the step)
        if kind == "SGD":
            assert torch.equal(hip.p[seg[ZERO_G]:seg[ZERO_G + 1]], p0[seg[ZERO_G]:seg[ZERO_G + 1]])
    assert float(hip.coef[0]) < 1.0 and float(hip.coef[1]) < 1.0 and float(hip.coef[2]) == 1.0
    live = torch.ones(hip.total, dtype=torch.bool, device=cuda)
    live[seg[SKIPPED]:seg[SKIPPED + 1]] = False
    assert torch.equal(hip.shadow[live], hip.p[live].to(torch.bfloat16))


def test_lion_sign_rule_on_large_tensors(lib, cuda):
    """Two 2M-element tensors of uniform(-1, 1) parameters and gradients that change sign between steps, 6 steps, no clip to speak of:
    outside the excused set the kernel and the fp32 restatement agree to < 1e-6, the set stays under 1e-4 of each tensor (the fp64
    and fp32 restatements alone: <= 1.7e-6 per step), and the moment, which no sign enters, agrees everywhere."""
    n = 2 * 1024 * 1024
    seg_t = torch.tensor([0, n, 2 * n], dtype=torch.int64, device=cuda)
    p = _hu(2 * n, 11, cuda)
    m = torch.zeros_like(p)
    p32, m32, p64, m64 = p.clone(), m.clone(), p.double(), m.double()
    excused = torch.zeros(2 * n, dtype=torch.bool, device=cuda)
    for step in range(6):
        g = _hu(2 * n, 20 + step, cuda) * (1.0 + 0.2 * step)
        gk = g.clone()
        _lib.check(lib.hct_lion_step(p.data_ptr(), gk.data_ptr(), m.data_ptr(), seg_t.data_ptr(), None, None, 2, 2 * n, HP["lr"], HP["beta1"], HP["beta2"],
                                     HP["weight_decay"], None, _st()), "lion")
        assert torch.equal(gk, g)  # no coefficient: the gradient is not written
        m_before = m64.clone()
        R.lion_step_(p32, g, m32, HP["lr"], HP["weight_decay"], HP["beta1"], HP["beta2"])
        c64 = R.lion_step_(p64, g.double(), m64, HP["lr"], HP["weight_decay"], HP["beta1"], HP["beta2"])
        new = R.lion_excused(c64, m_before, g.double(), HP["beta1"])
        excused |= new
        for h in (slice(0, n), slice(n, 2 * n)):
            keep = ~excused[h]
            share = 1.0 - float(keep.float().mean())
            print(f"step {step}: excused share {share:.2e} (this step {float(new[h].float().mean()):.2e})")
            assert share <= LION_CAP
            assert rel_err(p[h][keep], p32[h][keep]) < 1e-6 and rel_err(p[h][keep], p64[h][keep]) < 1e-6
            assert rel_err(m[h], m32[h]) < 1e-6


@pytest.mark.parametrize("kind", R.KINDS)
def test_kernels_are_bit_reproducible(lib, cuda, kind):
    """Every kernel twice from the same inputs: bit-identical outputs, Lamb's folds and diagnostics included."""
    runs = []
    for _ in range(2):
        f = _Flat(lib, kind, cuda)
        for step in range(3):
            f.step(_inputs(cuda, step))
        torch.cuda.synchronize()
        runs.append([t.clone() for t in f.everything()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- the MAE step ----------------------------------------------------------------------------------------------------------------
def _config(kind, sched, hp):
    from headct_foundation_amd.cfgnode import CfgNode
    c = CfgNode()
    c.MODEL = CfgNode(); c.MODEL.NAME = "mae"
    c.TRAIN = CfgNode()
    c.TRAIN.GRAD_CLIP, c.TRAIN.OPTIMIZER, c.TRAIN.SCHEDULER = hp["grad_clip"], kind, sched
    c.TRAIN.WEIGHT_DECAY, c.TRAIN.BETA1, c.TRAIN.BETA2, c.TRAIN.MOMENTUM = hp["weight_decay"], hp["beta1"], hp["beta2"], hp["momentum"]
    return c


def _build(kind, sched, hp, model):
    from headct_foundation_amd.lr_sched import get_lr_scheduler
    from headct_foundation_amd.optim import get_optimizer
    cfg = _config(kind, sched, hp)
    opt = get_optimizer(cfg, hp["base_lr"], [model])
    return cfg, opt, get_lr_scheduler(cfg, opt, hp["warmup"], hp["total"], hp["min_lr"])


@pytest.mark.parametrize("kind,sched", R.curve_runs())
def test_mae_loss_curve_through_train_one_epoch_vs_reference(lib, cuda, monkeypatch, kind, sched):
    """engine_pretrain_mae.train_one_epoch on `micro` (fp32 mode, per-tensor clip) with every new optimizer under every schedule
    (and AdamW under the two new schedules): the 4-step loss curve against the reference's own train_one_epoch (fixture) at the
    1e-3 relative bar of DESIGN.md 3, the rates to 1e-9.  The fourth loss has seen three updates, the third of them at a rate that
    differs between the schedules: updated weights, shadow and transposed copies reach the next forward."""
    import engine_pretrain_mae as E
    fx = next(c for c in load_golden("optimizers")["curves"] if c["optimizer"] == kind and c["scheduler"] == sched)
    hp, cfg = fx["hp"], O.CONFIGS[fx["config"]]
    model = build_hip_model(cfg, O.make_params(cfg, fx["seed"]), cuda, "fp32", full_pred=False)
    ecfg, opt, sch = _build(kind, sched, hp, model)
    batches = [O.make_volume(cfg, fx["batch"], fx["seed"] + 10 + i) for i in range(fx["steps"])]
    noises = iter([O.make_noise(cfg, fx["batch"], fx["seed"] + 10 + i).to(cuda) for i in range(fx["steps"])])
    monkeypatch.setattr(torch, "rand", lambda *a, **k: next(noises).clone())  # the forward's only draw (mae.py:206)
    monkeypatch.setenv("HCT_SYNC_LOSS", "1")
    lines, lrs = [], []

    class Tap(logging.Handler):
        def emit(self, record):
            lines.append(record.getMessage())
    log = logging.getLogger(f"optim-{kind}-{sched}")
    log.setLevel(logging.INFO); log.propagate = False
    log.addHandler(Tap())
    real_step = sch.step

    def spy(*a, **k):
        lrs.append(opt.param_groups[0]["lr"])
        return real_step(*a, **k)
    sch.step = spy
    stats = E.train_one_epoch(ecfg, model, batches, opt, sch, 0, 1, logger=log, device=cuda)
    losses = [float(l.split("Loss:")[1]) for l in lines if "Loss:" in l]
    print(kind, sched, "hip", losses, "reference", fx["logged_losses"], "avg", stats["loss"], fx["avg_loss"])
    assert np.allclose(lrs, fx["lrs"], rtol=1e-9, atol=0)
    assert len(losses) == fx["steps"] and all(abs(a - b) <= 1e-3 * abs(b) for a, b in zip(losses, fx["logged_losses"])), (losses, fx["logged_losses"])
    assert abs(stats["loss"] - fx["avg_loss"]) <= 1e-3 * abs(fx["avg_loss"])
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("kind,sched", [r for r in R.curve_runs() if r[0] != "AdamW"])
def test_mae_update_vs_restatement_fed_the_hip_gradients(lib, cuda, kind, sched):
    """A hand-written step loop on `micro` (fp32 mode, per-tensor clip deferred to the optimizer kernel): after every step the
    written-back (clipped) .grad of every parameter is applied by the restatement to ITS OWN running parameters / state at the
    scheduler's rate, and parameters and state are compared -- SGD and Lamb per tensor at 1e-6 times the number of steps so far,
    Lion per element by the sign rule with the cap over the model as a whole (1e-4 of 115 424 elements = 11)."""
    from headct_foundation_amd.optim import clip_gradients
    cfg = O.CONFIGS["micro"]
    hp = dict(R.CURVE_HP, base_lr=R.CURVE_LR[kind])
    params = O.make_params(cfg, 0)
    model = build_hip_model(cfg, params, cuda, "fp32", full_pred=False)
    _, opt, sch = _build(kind, sched, hp, model)
    named = dict(model.named_parameters())
    start = {k: v.detach().clone() for k, v in named.items()}
    mine = {k: v.detach().clone() for k, v in named.items() if v.requires_grad}
    mine64 = {k: v.double() for k, v in mine.items()}
    state = {k: R.new_state(kind, v) for k, v in mine.items()}
    state64 = {k: R.new_state(kind, v) for k, v in mine64.items()}
    excused = {k: torch.zeros_like(v, dtype=torch.bool) for k, v in mine.items()}
    total = sum(v.numel() for v in named.values())
    for step in range(4):
        opt.zero_grad()
        loss, _, _ = model(O.make_volume(cfg, 2, 10 + step).to(cuda), noise=O.make_noise(cfg, 2, 10 + step).to(cuda))
        loss.backward()
        clip_gradients(model, hp["grad_clip"])
        lr = opt.param_groups[0]["lr"]
        assert lr == pytest.approx(hp["base_lr"] * R.factor(sched, step, hp["warmup"], hp["total"], hp["base_lr"], hp["min_lr"]), rel=1e-12, abs=0)
        opt.step()
        sch.step()
        worst = 0.0
        for k, p in named.items():
            if not p.requires_grad:
                assert p.grad is None and torch.equal(p.detach(), start[k]), k
                continue
            g = p.grad.detach().clone()  # what the optimizer kernel left: the clipped gradient
            assert float(g.norm()) <= hp["grad_clip"] * (1 + 1e-5)
            R.apply_(kind, mine[k], g, state[k], lr, hp)
            if kind == "Lion":
                m_before = state64[k]["exp_avg"].clone()
                c64 = R.apply_(kind, mine64[k], g.double(), state64[k], lr, hp)
                excused[k] |= R.lion_excused(c64, m_before, g.double(), hp["beta1"])
                keep = ~excused[k]
                assert torch.equal(p.detach()[keep], mine[k][keep]) or rel_err(p.detach()[keep], mine[k][keep]) < 1e-6 * (step + 1), (step, k)
            else:
                e = rel_err(p.detach(), mine[k])
                worst = max(worst, e)
                assert e < 1e-6 * (step + 1), (step, k, e)
            got = opt.state[p]
            for key in R.STATE_KEYS[kind]:
                ref = state[k][key]
                assert rel_err(got[key], ref) < 1e-6 * (step + 1) or float(ref.abs().max()) == 0.0 and not got[key].any(), (step, k, key)
            if kind == "Lamb":
                assert got["step"] == step + 1
                for key in ("weight_norm", "adam_norm", "trust_ratio"):
                    a, b = float(got[key]), float(state[k][key])
                    assert abs(a - b) <= 1e-6 * (step + 1) * abs(b), (step, k, key, a, b)
        n_ex = sum(int(e.sum()) for e in excused.values())
        print(f"{kind}/{sched} step {step}: lr {lr:.3e} worst per-tensor relative error {worst:.2e}, excused elements {n_ex} of {total}")
        assert total == 115424 and n_ex <= int(LION_CAP * total)


@pytest.mark.parametrize("kind,lr", [("Lion", 3e-4), ("SGD", 0.1), ("Lamb", 1e-2)])
def test_bf16_loss_curve_vs_restatement(lib, cuda, kind, lr):
    """test_bf16_loss_curve_vs_oracle's recipe (`tiny`, B = 2, bf16 storage + MFMA, 20 steps of zero_grad / forward / backward / clip
    3.0 / step / cosine-warmup rate) with each new optimizer, against the fp32 restatement on the same volumes and masks: every
    step's loss within 5e-3 relative.  The rates are such that the fp32 curve falls by more than 10 %."""
    from headct_foundation_amd.optim import clip_gradients
    cfg = O.CONFIGS["tiny"]
    hp = dict(base_lr=lr, min_lr=lr * 1e-3, warmup=4, total=60, weight_decay=5e-3, beta1=0.9, beta2=0.95, momentum=0.9, grad_clip=3.0)
    params = O.make_params(cfg, 7)
    st = R.TrainState({k: v.clone() for k, v in params.items()})
    model = build_hip_model(cfg, params, cuda, "bf16", full_pred=False).train()
    _, opt, sch = _build(kind, "cosine", hp, model)
    hip, ref = [], []
    for i in range(20):
        x, noise = O.make_volume(cfg, 2, 100 + i % 4), O.make_noise(cfg, 2, 200 + i)
        ref.append(R.train_step(cfg, st, x, noise, kind, "cosine", **hp)[0])
        opt.zero_grad()
        loss, _, _ = model(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        clip_gradients(model, hp["grad_clip"])
        opt.step(); sch.step()
        hip.append(float(loss.detach()))
    rel = [abs(a - b) / abs(b) for a, b in zip(hip, ref)]
    print(f"\n{kind}: step  hip-bf16   restatement-fp32   rel")
    for i in range(20):
        print(f"   {i:3d}  {hip[i]:.5f}   {ref[i]:.5f}   {rel[i]:.2e}")
    assert ref[0] - min(ref) > 0.1 * ref[0], "the reference curve is flat: raise the learning rate"
    assert max(rel) < 5e-3, (max(rel), rel.index(max(rel)))


# ---- downstream fine-tuning ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("case", ["linear", "attentive", "lora"])
def test_finetune_steps_vs_restatement(lib, cuda, kind, case):
    """Two downstream steps (backbone at lr, head at 100 x lr, total-norm clip 1.0 on each, as main_downstream.py / engine_downstream.py
    do) with each optimizer, plain with the linear and the attentive head and with TRAIN.LORA's freezing rule: frozen parameters and
    their state keep their bits, trainable ones match the restatement fed the HIP path's own gradients (1e-6 per step; Lion by the
    sign rule, cap over backbone + head), the bf16 shadow is the rounded parameter."""
    from headct_foundation_amd import AttentionClassifier, LinearClassifier, cross_entropy
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.misc import set_requires_grad_false
    from headct_foundation_amd.optim import clip_grad_norm_, make_optimizer
    torch.manual_seed(4)
    lora = case == "lora"
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
                      compute_dtype="bf16", lora=lora)
    sd = vit.state_dict()
    for n in sd:
        if n in ("cls_token", "register_tokens") or "lora" in n:
            sd[n] = torch.randn(sd[n].shape) * (0.5 if "token" in n else 0.05)
    vit.load_state_dict(sd, strict=True)
    vit = vit.to(cuda).train()
    if lora:
        set_requires_grad_false(vit, lora=True)
    cls = (AttentionClassifier(48, 2, num_heads=12, compute_dtype="bf16") if case == "attentive" else LinearClassifier(48, 2, feature_grad=True)).to(cuda).train()
    lr = {"Lion": 1e-4, "SGD": 1e-3, "Lamb": 1e-3}[kind]
    hp = dict(weight_decay=0.04, beta1=0.9, beta2=0.95, momentum=0.9)
    mods = [(vit, make_optimizer(kind, vit, lr, betas=(0.9, 0.95), weight_decay=0.04, momentum=0.9), lr),
            (cls, make_optimizer(kind, cls, 100 * lr, betas=(0.9, 0.95), weight_decay=0.04, momentum=0.9), 100 * lr)]
    x = (torch.rand(8, 3, 24, 24, 24) * torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0]).view(-1, 1, 1, 1, 1)).to(cuda)
    tg = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1], device=cuda)
    start = [{k: v.detach().clone() for k, v in m.named_parameters()} for m, _, _ in mods]
    mine = [{k: v.clone() for k, v in s.items()} for s in start]
    mine64 = [{k: v.double() for k, v in s.items()} for s in start]
    state = [{k: R.new_state(kind, v) for k, v in s.items()} for s in mine]
    state64 = [{k: R.new_state(kind, v) for k, v in s.items()} for s in mine64]
    excused = [{k: torch.zeros_like(v, dtype=torch.bool) for k, v in s.items()} for s in start]
    total = sum(v.numel() for s in start for v in s.values())
    for step in range(2):
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
                        assert all(not o.state[p][key].any() for key in R.STATE_KEYS[kind])
                    continue
                assert torch.equal(p.grad, grads[j][k])  # the clip was applied in place: nothing is written back by the optimizer
                R.apply_(kind, mine[j][k], grads[j][k], state[j][k], lr_j, hp)
                if kind == "Lion":
                    m_before = state64[j][k]["exp_avg"].clone()
                    c64 = R.apply_(kind, mine64[j][k], grads[j][k].double(), state64[j][k], lr_j, hp)
                    excused[j][k] |= R.lion_excused(c64, m_before, grads[j][k].double(), hp["beta1"])
                    keep = ~excused[j][k]
                    assert torch.equal(p.detach()[keep], mine[j][k][keep]) or rel_err(p.detach()[keep], mine[j][k][keep]) < 1e-6 * (step + 1), (case, k)
                else:
                    assert rel_err(p.detach(), mine[j][k]) < 1e-6 * (step + 1), (case, k, rel_err(p.detach(), mine[j][k]))
                for key in R.STATE_KEYS[kind]:
                    ref = state[j][k][key]
                    assert rel_err(o.state[p][key], ref) < 1e-6 * (step + 1) or float(ref.abs().max()) == 0.0, (case, k, key)
        assert torch.equal(vit._flat_bf16, vit._flat.to(torch.bfloat16))
    frozen = {k for k, p in vit.named_parameters() if not p.requires_grad}
    n_ex = sum(int(e.sum()) for d in excused for e in d.values())
    print(f"{kind}/{case}: excused {n_ex} of {total} elements, {len(frozen)} frozen tensors")
    assert bool(frozen) == lora and n_ex <= int(LION_CAP * total)
    for name, off, numel, *_ in vit._layout:  # a frozen segment's state keeps its (zero) bits
        if name in frozen:
            assert all(not mods[0][1]._flat_buffer(key)[off:off + numel].any() for key in R.STATE_KEYS[kind]), name
    for j, (m, _, _) in enumerate(mods):
        assert any(not torch.equal(p.detach(), start[j][k]) for k, p in m.named_parameters() if p.requires_grad)


# ---- DINO ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Lion", "SGD", "Lamb", "AdamW"])
def test_dino_iteration_and_merged_state_dict(lib, cuda, kind):
    """One DINO iteration on a tiny student with DinoOptimizer(kind=...): the merged state dict (one dict over backbone + head
    parameters, the kind's own keys) loads into a fresh DinoOptimizer over a copy of the student, and a second iteration from both
    gives the same bits."""
    from headct_foundation_amd.dino import DINOLoss, DinoOptimizer
    from headct_foundation_amd.dino_model import DINOHead, MultiCropWrapper, ViTBackbone
    torch.manual_seed(6)

    def mk():
        b = ViTBackbone(img_size=24, patch_size=12, in_chans=3, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3)  # the tiny plumbing yaml
        return MultiCropWrapper(b, DINOHead(48, 512, hidden_dim=64, bottleneck_dim=32)).to(cuda)
    student, twin, teacher = mk(), mk(), mk()
    twin.load_state_dict(student.state_dict())
    teacher.load_state_dict(student.state_dict())
    crops = [torch.rand(2, 3, 24, 24, 24, device=cuda) for _ in range(4)]
    crit = DINOLoss(512, 4, 0.04, 0.04, 30, 200).to(cuda)
    with torch.no_grad():
        t_out = teacher(crops[:2])['dino_output'].float()

    def iteration(model, opt):
        opt.zero_grad()
        crit.center.zero_()
        loss = crit(model(crops)['dino_output'].float(), t_out, 0)
        loss.backward()
        opt.param_groups[0]["weight_decay"] = 0.05  # what the weight-decay schedule does every iteration
        opt.step()
        return float(loss.detach())

    mk_opt = lambda m: DinoOptimizer(m, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.04, kind=kind, momentum=0.9)
    opt = mk_opt(student)
    l0 = iteration(student, opt)
    assert np.isfinite(l0)
    sd = opt.state_dict()
    nb = len(list(student.backbone.parameters()))
    assert sd["param_groups"][0]["params"] == list(range(len(list(student.parameters())))) and max(sd["state"]) >= nb
    keys = {"AdamW": {"step", "exp_avg", "exp_avg_sq"}, "Lion": {"exp_avg"}, "SGD": {"momentum_buffer"},
            "Lamb": {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}}[kind]
    assert all(set(v) == keys for v in sd["state"].values())
    twin.load_state_dict(student.state_dict())
    opt2 = mk_opt(twin)
    opt2.load_state_dict(sd)
    sd2 = opt2.state_dict()
    for i, entry in sd["state"].items():
        for k, v in entry.items():
            assert torch.equal(torch.as_tensor(sd2["state"][i][k]).cpu().float(), torch.as_tensor(v).cpu().float()), (i, k)
    l1, l2 = iteration(student, opt), iteration(twin, opt2)
    assert l1 == l2
    for (n, a), (_, b) in zip(student.named_parameters(), twin.named_parameters()):
        assert torch.equal(a, b), n
    assert any(not torch.equal(a, b) for (_, a), (_, b) in zip(student.named_parameters(), teacher.named_parameters()))


# ---- resume ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sched", [("Lion", "poly"), ("SGD", "constant"), ("Lamb", "poly")])
def test_resume_reproduces_uninterrupted_run(lib, cuda, tmp_path, kind, sched):
    """save_checkpoint -> fresh model / optimizer / scheduler -> load_optimizer -> continue == the uninterrupted run, bit for bit."""
    from headct_foundation_amd import MaskedAutoencoderViT
    from headct_foundation_amd.misc import load_optimizer, save_checkpoint
    from headct_foundation_amd.optim import clip_gradients
    cfg = O.CONFIGS["micro"]
    hp = dict(R.CURVE_HP, base_lr=R.CURVE_LR[kind], warmup=2, total=10)

    def fresh():
        m = MaskedAutoencoderViT(**cfg.ctor_kwargs(), compute_dtype="fp32")
        m.load_state_dict(O.make_params(cfg, 0))
        m = m.to(cuda)
        _, opt, sch = _build(kind, sched, hp, m)
        return m, opt, sch

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


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def _epoch_losses(log):
    return [float(l.split("Loss:")[1].split()[0]) for l in log.splitlines() if "] " in l and "Loss:" in l and "Epoch" in l]


@pytest.mark.parametrize("entry,kind,sched", [("mae", "Lion", "poly"), ("dino", "Lamb", "constant"), ("downstream", "SGD", "poly")])
def test_entry_points_accept_the_new_values(cuda, tmp_path, entry, kind, sched):
    """--optimizer / --scheduler through the three entry points on their tiny plumbing configurations: the run completes and writes a
    checkpoint whose optimizer state has the kind's keys."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    with socket.socket() as sock:  # a port nobody holds right now, not a fixed one another job on the machine may be using
        sock.bind(("127.0.0.1", 0))
        port = str(sock.getsockname()[1])
    run = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1", "--master-port", port]
    out = ["MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log")]
    if entry == "mae":
        cmd = run + [os.path.join(ROOT, "main_pretrain_mae.py"), "--local_rank", "0", "--model_name", "mae", "--batch_size", "2", "--max_epochs", "2",
                     "--base_lr", "3e-4", "--cfg", os.path.join(ROOT, "configs/mae/mae_tiny_plumbing.yaml"), "--optimizer", kind, "--scheduler", sched,
                     "--weight_decay", "5e-3", "--grad_clip", "3.0", "--opts"] + out + ["OUTPUT", str(tmp_path / "json")]
        ckpt = "latest_mae_tiny.pt"
    elif entry == "dino":
        cmd = run + [os.path.join(ROOT, "main_pretrain_dino.py"), "--local_rank", "0", "--model_name", "dino", "--batch_size", "2", "--max_epochs", "2",
                     "--base_lr", "5e-3", "--cfg", os.path.join(ROOT, "configs/dino/dino_tiny_plumbing.yaml"), "--optimizer", kind, "--scheduler", sched,
                     "--opts"] + out + ["OUTPUT", str(tmp_path / "json")]
        ckpt = "last_dino_tiny.pt"
    else:
        cfg = tmp_path / "cfg.yaml"
        cfg.write_text("MODEL:\n  NAME: vit\n")
        opts = ["DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12", "VIT.HIDDEN_SIZE", "48",
                "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1", "MODEL.SAVE_NAME", "ft.pt", "PREDS_SAVE_NAME", "run"]
        cmd = run + [os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--classifier", "linear", "--batch_size", "4",
                     "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-3", "--optimizer", kind, "--scheduler", sched, "--opts"] + opts + out
        ckpt = None
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "nan" not in log.lower().replace("nanosecond", "")
    if ckpt:
        ck = torch.load(tmp_path / "ckpt" / ckpt, map_location="cpu", weights_only=True)
        keys = {"Lion": {"exp_avg"}, "SGD": {"momentum_buffer"}, "Lamb": {"step", "exp_avg", "exp_avg_sq", "weight_norm", "adam_norm", "trust_ratio"}}[kind]
        assert set(ck["optimizer"]["state"][0].keys()) == keys
        assert ck["scheduler"]["lr_lambdas"] == [None]
