"""GPU: the RMSNorm path (MAE.NORM_LAYER: rmsnorm) -- kernels through the C ABI against torch autograd in fp64, the MAE and the
encoder-only models against the fixture made from the reference (tests/golden/rmsnorm.json) and the restatement
(tests/rmsnorm_ref.py), the plan's exact re-formulations, training curves, and the entry points.

Tolerances are the project's bars for the same arithmetic: fp32 1e-3 relative on loss, activations, prediction
and every gradient; bf16 gradients 2e-2 per tensor against the restatement with bf16-rounded storage; loss curves 5e-3 per step."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import rmsnorm_ref as R
from tests.util import grads_by_name, load_golden, rel_err, sample_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [("micro", 2, 0), ("yaml_cut", 2, 1), ("tiny", 2, 0), ("vitb_cut", 2, 0)]


def _dt(t):
    from headct_foundation_amd import _lib
    return _lib.dtype_code(t)


def _st():
    from headct_foundation_amd import _lib
    return _lib.stream_ptr()


def _build(cfg, params, device, dtype="fp32", full_pred=True):
    from headct_foundation_amd import MaskedAutoencoderViT, RMSNorm
    m = MaskedAutoencoderViT(**cfg.ctor_kwargs(), norm_layer=RMSNorm, compute_dtype=dtype)
    m.load_state_dict(params, strict=True)
    m.full_pred = full_pred
    return m.to(device).train()


def _step(model, x, noise):
    for p in model.parameters():
        p.grad = None
    loss, a, b = model(x, noise=noise)
    assert a is None and b is None
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), grads_by_name(model)


def _check_grads(grads, want, tol, abs_tol=1e-3):
    """Every gradient tensor at `tol` (relative L2); the qkv bias, whose K-third is mathematically zero, absolutely."""
    frozen = {"decoder_pos_embed"}
    assert set(grads) == set(want) and not (set(grads) & frozen)
    worst = max((rel_err(grads[k], want[k]), k) for k in grads if not k.endswith("qkv.bias"))
    print("worst gradient", worst)
    assert worst[0] < tol, worst
    for k in grads:
        if k.endswith("qkv.bias"):
            assert (grads[k] - want[k]).abs().max() < 1e-6 + abs_tol * want[k].abs().max(), k


# ---- 5. kernels --------------------------------------------------------------------------------------------------------------
def _rms_ref(x, gamma, dy, eps=1e-6):
    xr, gr = x.double().clone().requires_grad_(True), gamma.double().clone().requires_grad_(True)
    y = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps) * gr
    if dy is not None:
        (y * dy.double()).sum().backward()
    return y.detach(), xr.grad, gr.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,D", [(7, 48), (5, 192), (217, 768), (110, 768), (1030, 1024), (4099, 768)])
def test_rmsnorm_kernels_vs_fp64_autograd(lib, cuda, rows, D, dtype):
    """(The sentinel 768 is exact in bfloat16.)  hct_rmsnorm_fwd / hct_rmsnorm_bwd: y, rstd, dx (+ residual gradient, in place), shadow, dgamma, column sum; row counts that are
    no multiple of the 4 waves of a workgroup (and more rows than the backward has waves); outputs pre-filled with a sentinel;
    with and without dres / dcolsum / shadow; a repeated call is bit-identical."""
    from headct_foundation_amd import _lib
    g = torch.Generator().manual_seed(rows * 31 + D)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.3).to(cuda)
    gamma = (1 + 0.1 * torch.randn(D, generator=g)).to(cuda)
    dy = torch.randn(rows, D, generator=g).to(cuda).to(dtype)
    dres = torch.randn(rows, D, generator=g).to(cuda)
    y_ref, dx_ref, dg_ref = _rms_ref(x, gamma, dy)
    lo = 4e-3 if dtype == torch.bfloat16 else 1e-5  # one bf16 rounding of an output / fp32 arithmetic
    y = torch.full((rows, D), 768.0, dtype=dtype, device=cuda)
    rstd = torch.full((rows,), 768.0, device=cuda)
    _lib.check(lib.hct_rmsnorm_fwd(x.data_ptr(), gamma.data_ptr(), rows, D, 1e-6, y.data_ptr(), _dt(y), rstd.data_ptr(), _st()), "rms fwd")
    assert rel_err(y, y_ref) < lo
    assert rel_err(rstd, torch.rsqrt(x.double().pow(2).mean(-1) + 1e-6)) < 1e-6
    ws = torch.empty(lib.hct_rmsnorm_bwd_workspace_bytes(rows, D), dtype=torch.uint8, device=cuda)
    assert ws.numel() == lib.hct_layernorm_bwd_workspace_bytes(rows, D)
    for with_dres in (True, False):
        for with_extra in (True, False):  # shadow + column sum
            outs = []
            for _ in range(2):
                dx = dres.clone() if with_dres else torch.full((rows, D), 768.0, device=cuda)
                shadow = torch.full((rows, D), 768.0, dtype=dtype, device=cuda)
                dg, dc = torch.full((D,), 768.0, device=cuda), torch.full((D,), 768.0, device=cuda)
                _lib.check(lib.hct_rmsnorm_bwd(dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                               dx.data_ptr() if with_dres else None, rows, D, dx.data_ptr(),
                                               shadow.data_ptr() if with_extra else None, _dt(shadow), dg.data_ptr(),
                                               dc.data_ptr() if with_extra else None, ws.data_ptr(), ws.numel(), _st()), "rms bwd")
                outs.append((dx, shadow, dg, dc))
            assert all(torch.equal(a, b) for a, b in zip(*outs)), "hct_rmsnorm_bwd is not bit-reproducible"
            dx, shadow, dg, dc = outs[0]
            want = dx_ref + (dres.double() if with_dres else 0)
            assert rel_err(dx, want) < 1e-5 and rel_err(dg, dg_ref) < 1e-5
            if with_extra:
                assert rel_err(shadow, want) < lo and rel_err(dc, want.sum(0)) < 1e-4
            else:  # untouched
                assert bool((shadow.float() == 768.0).all()) and bool((dc == 768.0).all())
    # fp32 dy with a bf16 shadow and the reverse (the two mixed instantiations)
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    dx, shadow, dg = torch.empty(rows, D, device=cuda), torch.empty(rows, D, dtype=other, device=cuda), torch.empty(D, device=cuda)
    _lib.check(lib.hct_rmsnorm_bwd(dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), None, rows, D, dx.data_ptr(),
                                   shadow.data_ptr(), _dt(shadow), dg.data_ptr(), None, ws.data_ptr(), ws.numel(), _st()), "rms bwd mixed")
    assert rel_err(dx, dx_ref) < 1e-5 and rel_err(shadow, dx_ref) < (4e-3 if other == torch.bfloat16 else 1e-5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_rmsnorm_fwd_generic_path_and_argument_checks(lib, cuda, dtype):
    """D = 1280 > 1024 takes the multi-pass forward; the backward refuses it; D % 4 != 0 and a small workspace are refused."""
    from headct_foundation_amd import _lib
    rows, D = 37, 1280
    g = torch.Generator().manual_seed(5)
    x, gamma = torch.randn(rows, D, generator=g).to(cuda), (1 + 0.1 * torch.randn(D, generator=g)).to(cuda)
    y, rstd = torch.full((rows, D), 768.0, dtype=dtype, device=cuda), torch.empty(rows, device=cuda)
    _lib.check(lib.hct_rmsnorm_fwd(x.data_ptr(), gamma.data_ptr(), rows, D, 1e-6, y.data_ptr(), _dt(y), rstd.data_ptr(), _st()), "rms fwd")
    assert rel_err(y, _rms_ref(x, gamma, None)[0]) < (4e-3 if dtype == torch.bfloat16 else 1e-5)
    ws = torch.empty(lib.hct_rmsnorm_bwd_workspace_bytes(rows, D), dtype=torch.uint8, device=cuda)
    dy, dx, dg = torch.zeros(rows, D, dtype=dtype, device=cuda), torch.empty(rows, D, device=cuda), torch.empty(D, device=cuda)
    args = lambda d, nbytes: (dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), None, rows, d, dx.data_ptr(), None, 0,
                              dg.data_ptr(), None, ws.data_ptr(), nbytes, _st())
    assert lib.hct_rmsnorm_bwd(*args(D, ws.numel())) != 0 and b"1024" in lib.hct_last_error_string()
    assert lib.hct_rmsnorm_bwd(*args(770, ws.numel())) != 0
    assert lib.hct_rmsnorm_bwd(*args(768, 16)) != 0 and b"workspace" in lib.hct_last_error_string()
    assert lib.hct_rmsnorm_fwd(x.data_ptr(), gamma.data_ptr(), rows, 770, 1e-6, y.data_ptr(), _dt(y), rstd.data_ptr(), _st()) != 0


@pytest.mark.parametrize("D", [48, 768])
def test_rmsnorm_bwd_mapped_equals_plain_on_scattered_matrix(lib, cuda, D):
    """The residual gradient read through a row map with -1 entries == the plain call on the scattered matrix, bit for bit."""
    from headct_foundation_amd import _lib
    M, Mc = 653, 401
    g = torch.Generator().manual_seed(D)
    x, dy = torch.randn(M, D, generator=g).to(cuda), torch.randn(M, D, generator=g).to(cuda).bfloat16()
    gamma, dres_c = torch.randn(D, generator=g).to(cuda), torch.randn(Mc, D, generator=g).to(cuda)
    rows = torch.randperm(M, generator=g)[:Mc]
    inv = torch.full((M,), -1, dtype=torch.int32)
    inv[rows] = torch.arange(Mc, dtype=torch.int32)
    inv = inv.to(cuda)
    dres_full = torch.zeros(M, D, device=cuda)
    dres_full[rows.to(cuda)] = dres_c
    rstd = torch.rsqrt(x.pow(2).mean(-1) + 1e-6)
    ws = torch.empty(lib.hct_rmsnorm_bwd_workspace_bytes(M, D), dtype=torch.uint8, device=cuda)
    outs = []
    for mapped in (False, True):
        dx, shadow = torch.empty(M, D, device=cuda), torch.empty(M, D, dtype=torch.bfloat16, device=cuda)
        dg, dc = torch.empty(D, device=cuda), torch.empty(D, device=cuda)
        if mapped:
            _lib.check(lib.hct_rmsnorm_bwd_mapped(dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dres_c.data_ptr(),
                                                  inv.data_ptr(), M, D, dx.data_ptr(), shadow.data_ptr(), _dt(shadow), dg.data_ptr(), dc.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _st()), "rms bwd mapped")
        else:
            _lib.check(lib.hct_rmsnorm_bwd(dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dres_full.data_ptr(), M, D,
                                           dx.data_ptr(), shadow.data_ptr(), _dt(shadow), dg.data_ptr(), dc.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _st()), "rms bwd")
        outs.append((dx, shadow, dg, dc))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    _, dx_ref, dg_ref = _rms_ref(x, gamma, dy)
    assert rel_err(outs[1][0], dx_ref + dres_full.double()) < 1e-5 and rel_err(outs[1][2], dg_ref) < 1e-5
    # a mapped residual gradient that aliases the output is refused
    dx = outs[1][0]
    assert lib.hct_rmsnorm_bwd_mapped(dy.data_ptr(), _dt(dy), x.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), inv.data_ptr(), M, D,
                                      dx.data_ptr(), None, 0, outs[1][2].data_ptr(), None, ws.data_ptr(), ws.numel(), _st()) != 0


# ---- 6. the MAE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,seed", CASES)
def test_mae_fp32_vs_restatement_and_fixture(lib, cuda, name, batch, seed):
    cfg = O.CONFIGS[name]
    params = R.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    o_loss, o_pred, o_mask, o_grads, o_inter = R.forward_backward(cfg, params, x, noise, want_inter=True)
    model = _build(cfg, params, cuda, "fp32")
    loss, grads = _step(model, x.to(cuda), noise.to(cuda))
    tol = 1e-3
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < tol
    assert torch.equal(model.last_mask(batch).cpu(), o_mask)
    assert rel_err(model.last_pred(batch), o_pred) < tol
    keys = ["latent", "enc_in", "dec_in"] + [f"enc{i}.out" for i in range(cfg.encoder_depth)] + [f"dec{i}.out" for i in range(cfg.decoder_depth)]
    for key in keys:
        assert rel_err(model.activation(key, batch).float().view_as(o_inter[key]), o_inter[key]) < tol, key
    _check_grads(grads, o_grads, tol)
    if name in ("micro", "yaml_cut"):  # the reference's own outputs
        fx = load_golden("rmsnorm")["mae"][name]
        assert abs(loss - fx["loss"]) / abs(fx["loss"]) < tol
        got, want, l2, l2w = sample_of(model.last_pred(batch), fx["pred"])
        assert abs(l2 - l2w) / l2w < tol and torch.allclose(got, want, rtol=1e-3, atol=1e-4 * float(want.abs().max()))
        for k, entry in fx["act"].items():
            got, want, l2, l2w = sample_of(model.activation(k, batch).float(), entry)
            assert abs(l2 - l2w) / l2w < tol and torch.allclose(got, want, rtol=1e-3, atol=1e-4 * float(want.abs().max())), k
        assert set(fx["grads"]) == set(grads)
        for k, entry in fx["grads"].items():
            got, want, l2, l2w = sample_of(grads[k], entry)
            if k.endswith("qkv.bias"):
                assert (got - want).abs().max() < 1e-6 + 1e-3 * float(want.abs().max()), k
            else:
                assert abs(l2 - l2w) <= 1e-3 * l2w + 1e-9, k
                assert torch.allclose(got, want, rtol=2e-3, atol=2e-4 * float(want.abs().max()) + 1e-10), k


@pytest.mark.parametrize("name,batch,seed", CASES)
def test_mae_bf16_vs_bf16_storage_restatement(lib, cuda, name, batch, seed):
    """As test_model_gpu.test_bf16_gradients_vs_bf16_storage_oracle: loss 1e-3, pred 5e-3, per-tensor gradient L2 2e-2."""
    cfg = O.CONFIGS[name]
    params = R.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed), O.make_noise(cfg, batch, seed)
    o_loss, o_pred, o_mask, o_grads, _ = R.forward_backward(cfg, params, x, noise, emulate_bf16=True)
    model = _build(cfg, params, cuda, "bf16")
    loss, grads = _step(model, x.to(cuda), noise.to(cuda))
    assert abs(loss - float(o_loss)) / abs(float(o_loss)) < 1e-3
    assert torch.equal(model.last_mask(batch).cpu(), o_mask)
    assert rel_err(model.last_pred(batch), o_pred) < 5e-3
    _check_grads(grads, o_grads, 2e-2, abs_tol=2e-2)


# ---- 7. the exact re-formulations --------------------------------------------------------------------------------------------
def _same(a, b, tol):
    assert abs(a[0] - b[0]) <= tol * abs(b[0])
    assert set(a[1]) == set(b[1])
    for k, g in b[1].items():
        if k.endswith("qkv.bias"):
            assert (a[1][k] - g).abs().max() <= 1e-6 + tol * g.abs().max(), k
        else:
            assert rel_err(a[1][k], g) < tol, (k, rel_err(a[1][k], g))


@pytest.mark.parametrize("name,batch,seed", CASES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_compact_tail_on_off(lib, cuda, name, batch, seed, dtype):
    """Tolerances of test_model_gpu.test_compact_decoder_tail_vs_full_and_oracle: fp32 1e-5, bf16 2e-3 (summation order)."""
    cfg = O.CONFIGS[name]
    params = R.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed).to(cuda), O.make_noise(cfg, batch, seed).to(cuda)
    full = _step(_build(cfg, params, cuda, dtype, full_pred=True), x, noise)
    tail = _step(_build(cfg, params, cuda, dtype, full_pred=False), x, noise)
    _same(tail, full, 1e-5 if dtype == "fp32" else 2e-3)
    if dtype == "fp32":
        o_loss, _, _, o_grads, _ = R.forward_backward(cfg, params, x.cpu(), noise.cpu())
        assert abs(tail[0] - float(o_loss)) / abs(float(o_loss)) < 1e-3
        _check_grads(tail[1], o_grads, 1e-3)


@pytest.mark.parametrize("name,batch,seed", [("micro2", 2, 0), ("tiny", 3, 1), ("yaml_cut2", 2, 1)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_first_decoder_block_on_cat_rows_on_off(lib, cuda, name, batch, seed, dtype):
    """Tolerances of test_model_gpu.test_first_decoder_block_on_cat_rows_vs_every_row: fp32 1e-5, bf16 3e-3."""
    cfg = dataclasses.replace(O.CONFIGS[name[:-1]], decoder_depth=2) if name.endswith("2") else O.CONFIGS[name]
    assert cfg.decoder_depth >= 2
    params = R.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed).to(cuda), O.make_noise(cfg, batch, seed).to(cuda)
    out = {}
    for key in ("rows", "cat"):
        m = _build(cfg, params, cuda, dtype, full_pred=False)
        m.dec0_table = key == "cat"
        out[key] = _step(m, x, noise)
    _same(out["cat"], out["rows"], 1e-5 if dtype == "fp32" else 3e-3)
    if dtype == "fp32":
        o_loss, _, _, o_grads, _ = R.forward_backward(cfg, params, x.cpu(), noise.cpu())
        assert abs(out["cat"][0] - float(o_loss)) / abs(float(o_loss)) < 1e-3
        _check_grads(out["cat"][1], o_grads, 1e-3)


@pytest.mark.parametrize("name,batch,seed", [("tiny", 2, 0), ("vitb_cut", 2, 0)])
def test_queued_and_in_stage_weight_gradients(lib, cuda, name, batch, seed):
    """bf16 plans queue the weight gradients into grouped launches (hct_mae_plan_set_wgrad_defer); run in their stages instead, the
    same products go through the split-K kernel.  Same bf16 operands, fp32 accumulation in another order: the bf16 bar of the
    compact-tail switch for that effect (2e-3); the forward is untouched, so the loss is bit-equal."""
    cfg = O.CONFIGS[name]
    params = R.make_params(cfg, seed)
    x, noise = O.make_volume(cfg, batch, seed).to(cuda), O.make_noise(cfg, batch, seed).to(cuda)
    out = {}
    for defer in (1, 0):
        m = _build(cfg, params, cuda, "bf16", full_pred=False)
        plan = m._plan_for(batch)
        assert plan.lib.hct_mae_plan_set_wgrad_defer(plan.handle, defer, 0) == defer
        out[defer] = _step(m, x, noise)
    assert out[0][0] == out[1][0]
    _same(out[0], out[1], 2e-3)


# ---- 8. training curves --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch,seed", [("micro", 2, 0), ("yaml_cut", 2, 1)])
def test_train_curve_fp32_vs_reference_fixture(lib, cuda, name, batch, seed):
    """4 steps (per-tensor clip, HipAdamW, cosine LR) vs the reference's own train_one_epoch: the bars of
    test_model_gpu.test_train_curve_fp32_vs_golden."""
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import HipAdamW, clip_gradients
    tr = load_golden("rmsnorm")["mae"][name]["train"]
    hp = tr["hp"]
    cfg = O.CONFIGS[name]
    model = _build(cfg, R.make_params(cfg, seed), cuda, "fp32")
    opt = HipAdamW(model, lr=hp["base_lr"], weight_decay=hp["weight_decay"], betas=(hp["beta1"], hp["beta2"]))
    sched = get_cosine_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"])
    losses, lrs = [], []
    for i in range(tr["steps"]):
        opt.zero_grad()
        loss, _, _ = model(O.make_volume(cfg, batch, seed + 10 + i).to(cuda), noise=O.make_noise(cfg, batch, seed + 10 + i).to(cuda))
        loss.backward()
        clip_gradients(model, hp["grad_clip"])
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        losses.append(float(loss))
    print(name, "losses", losses, "reference", tr["logged_losses"])
    assert np.allclose(lrs, tr["lrs"], rtol=1e-9)
    assert np.allclose(losses, tr["logged_losses"], atol=2e-4), (losses, tr["logged_losses"])
    named = dict(model.named_parameters())
    assert set(named) == set(tr["params_after"])
    for k, entry in tr["params_after"].items():
        got, want, _, _ = sample_of(named[k], entry)
        assert torch.allclose(got, want, rtol=1e-4, atol=4 * hp["base_lr"] if k.endswith("qkv.bias") else 1e-5), k


def test_bf16_loss_curve_vs_restatement(lib, cuda):
    """24 optimizer steps on `tiny`, bf16, the module default (compact tail), LR raised so that the loss moves >= 10 %: every step
    within 5e-3 of the fp32 restatement's curve (the bars of test_model_gpu.test_bf16_loss_curve_vs_oracle)."""
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import HipAdamW, clip_gradients
    cfg, B, steps = O.CONFIGS["tiny"], 2, 24
    hp = dict(base_lr=2e-3, min_lr=2e-6, warmup=4, total=60, weight_decay=5e-3, grad_clip=3.0)
    params = R.make_params(cfg, 7)
    st32 = O.TrainState({k: v.clone() for k, v in params.items()})
    st16 = O.TrainState({k: v.clone() for k, v in params.items()})
    model = _build(cfg, params, cuda, "bf16", full_pred=False)
    opt = HipAdamW(model, lr=hp["base_lr"], weight_decay=hp["weight_decay"], betas=(0.9, 0.95))
    sched = get_cosine_schedule_with_warmup(opt, hp["warmup"], hp["total"], lr_end=hp["min_lr"])
    hip, ref32, ref16 = [], [], []
    for i in range(steps):
        x, noise = O.make_volume(cfg, B, 100 + i % 4), O.make_noise(cfg, B, 200 + i)
        ref32.append(R.train_step(cfg, st32, x, noise, **hp)[0])
        ref16.append(R.train_step(cfg, st16, x, noise, emulate_bf16=True, **hp)[0])
        opt.zero_grad()
        loss, _, _ = model(x.to(cuda), noise=noise.to(cuda))
        loss.backward()
        clip_gradients(model, hp["grad_clip"])
        opt.step()
        sched.step()
        hip.append(float(loss.detach()))
    for i in range(steps):
        print(f"   {i:3d}  hip {hip[i]:.5f}   fp32 {ref32[i]:.5f}   bf16-storage {ref16[i]:.5f}")
    assert ref32[0] - min(ref32) > 0.1 * ref32[0], "the reference curve is flat: raise the learning rate"
    rel = [abs(a - b) / abs(b) for a, b in zip(hip, ref32)]
    assert max(rel) < 5e-3, (max(rel), rel.index(max(rel)))
    assert sum(rel[-5:]) / 5 < 3e-3
    rel16 = [abs(a - b) / abs(b) for a, b in zip(hip, ref16)]
    assert max(rel16) < 3e-3, (max(rel16), rel16.index(max(rel16)))


# ---- 9. encoder-only -----------------------------------------------------------------------------------------------------------
def _vit_kwargs(lora, dtype):
    c = R.VIT_CASE
    return dict(in_chans=c["in_chans"], img_size=c["img_size"], patch_size=c["patch_size"], hidden_size=c["hidden_size"], mlp_dim=c["mlp_dim"],
                num_layers=c["num_layers"], num_heads=c["num_heads"], num_register_tokens=c["num_register_tokens"], qkv_bias=c["qkv_bias"],
                lora=lora, compute_dtype=dtype)


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 2e-2)])
def test_forward_only_vit_vs_reference_fixture(lib, cuda, dtype, tol, lora):
    from headct_foundation_amd import RMSNorm, ViT
    fx = load_golden("rmsnorm")["vit_lora" if lora else "vit"]
    c = fx["case"]
    params = R.vit_case_params({e["name"]: e["shape"] for e in fx["state_dict"]})
    model = ViT(**_vit_kwargs(lora, dtype), norm_layer=RMSNorm)
    model.load_state_dict(params, strict=True)
    model = model.to(cuda)
    x = R.vit_case_input()
    out, hidden = model(x.to(cuda))
    o_out, o_hidden = R.vit_forward(params, x, c["patch_size"], c["num_heads"], c["num_layers"])
    assert rel_err(out, o_out) < tol and len(hidden) == c["num_layers"]
    for a, b in zip(hidden, o_hidden):
        assert rel_err(a, b) < tol
    for t, entry in [(out, fx["out"])] + list(zip(hidden, fx["hidden"])):
        got, want, l2, l2w = sample_of(t, entry)
        assert abs(l2 - l2w) < tol * l2w
        if dtype == "fp32":
            assert torch.allclose(got, want, rtol=1e-3, atol=1e-4)
    # a volume of another size: the position table is resized for the call, the normalisation is unaffected by it
    x24 = torch.rand(2, 1, 24, 24, 24)
    out24, _ = model(x24.to(cuda))
    assert rel_err(out24, R.vit_forward(params, x24, c["patch_size"], c["num_heads"], c["num_layers"])[0]) < tol


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 2e-2)])
def test_backbone_tokens_and_gradients_vs_reference_fixture(lib, cuda, dtype, tol, lora):
    """ViTBackbone forward + backward of the fixture's scalar loss: tokens and EVERY trainable gradient against the reference's own
    ViT(norm_layer=RMSNorm) (fp32) and the restatement (bf16: with bf16-rounded storage), the LoRA rule applied where lora=True."""
    from headct_foundation_amd import RMSNorm
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.misc import set_requires_grad_false
    fx = load_golden("rmsnorm")["vit_lora" if lora else "vit"]
    c = fx["case"]
    params = R.vit_case_params({e["name"]: e["shape"] for e in fx["state_dict"]})
    model = ViTBackbone(**_vit_kwargs(lora, dtype), norm_layer=RMSNorm)
    model.load_state_dict(params, strict=True)
    model = model.to(cuda).train()
    if lora:
        set_requires_grad_false(model, lora=True)
    assert [n for n, p in model.named_parameters() if p.requires_grad] == fx["trainable"]
    x = R.vit_case_input()
    tok, _ = model(x.to(cuda))
    R.case_loss(tok.float()).backward()
    torch.cuda.synchronize()
    p = {k: v.clone().requires_grad_(k in fx["trainable"]) for k, v in params.items()}
    o_tok, _ = R.vit_forward(p, x, c["patch_size"], c["num_heads"], c["num_layers"], emulate_bf16=dtype == "bf16")
    R.case_loss(o_tok).backward()
    assert rel_err(tok, o_tok) < tol
    named = dict(model.named_parameters())
    errs = {}
    for k in fx["trainable"]:
        g, want = named[k].grad.float().cpu(), p[k].grad
        if k.endswith("qkv.bias"):
            assert (g - want).abs().max() < 1e-6 + tol * want.abs().max(), k
        else:
            errs[k] = rel_err(g, want)
    print("worst", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    assert max(errs.values()) < tol, sorted(errs.items(), key=lambda kv: -kv[1])[:3]
    assert all(named[k].grad is None for k in named if k not in fx["trainable"])
    if dtype == "fp32":
        got, want, l2, l2w = sample_of(tok, fx["out"])
        assert abs(l2 - l2w) < tol * l2w and torch.allclose(got, want, rtol=1e-3, atol=1e-4)
        for k, entry in fx["grads"].items():
            got, want, l2, l2w = sample_of(named[k].grad, entry)
            if k.endswith("qkv.bias"):
                assert (got - want).abs().max() < 1e-6 + 1e-3 * float(want.abs().max()), k
            else:
                assert abs(l2 - l2w) <= 1e-3 * l2w + 1e-9 and torch.allclose(got, want, rtol=2e-3, atol=2e-4 * float(want.abs().max()) + 1e-10), k


@pytest.mark.parametrize("lora", [False, True], ids=["plain", "lora"])
def test_full_finetune_step_vs_restatement(lib, cuda, lora):
    """One fine-tuning step through ViTBackbone + LinearClassifier, fp32, as test_finetune_gpu.test_full_finetune_step_vs_oracle
    (1e-3; the final norm's weight gradient, mathematically zero behind the head's BatchNorm, compared absolutely as there)."""
    from headct_foundation_amd import LinearClassifier, RMSNorm, cross_entropy
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.misc import set_requires_grad_false
    torch.manual_seed(4)
    tol, hidden, heads = 1e-3, 48, 3
    vit = ViTBackbone(in_chans=3, img_size=24, patch_size=12, hidden_size=hidden, mlp_dim=96, num_layers=2, num_heads=heads,
                      num_register_tokens=2, lora=lora, norm_layer=RMSNorm, compute_dtype="fp32")
    sd = vit.state_dict()
    for n in ("cls_token", "register_tokens"):
        sd[n] = torch.randn(sd[n].shape) * 0.5
    for k in sd:
        if k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * torch.randn(sd[k].shape)
        if k.endswith("lora_matrix_B"):
            sd[k] = 0.005 * torch.randn(sd[k].shape)
    vit.load_state_dict(sd, strict=True)
    vit = vit.to(cuda).train()
    if lora:
        set_requires_grad_false(vit, lora=True)
    cls = LinearClassifier(hidden, 2, feature_grad=True).to(cuda).train()
    x = torch.rand(8, 3, 24, 24, 24) * torch.tensor([0.5, 1.0, 2.0, 3.0, 4.0, 6.0, 8.0, 12.0]).view(-1, 1, 1, 1, 1)
    tg = torch.tensor([0, 1, 1, 0, 1, 0, 0, 1])
    loss = cross_entropy(cls(vit(x.to(cuda))[0]), tg.to(cuda))
    loss.backward()
    named = dict(vit.named_parameters())
    trainable = [k for k, v in named.items() if v.requires_grad]
    pv = {k: v.detach().cpu().float().clone().requires_grad_(k in trainable) for k, v in vit.state_dict().items()}
    ph = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in cls.named_parameters()}
    tok, _ = R.vit_forward(pv, x, 12, heads, 2)
    bn = torch.nn.BatchNorm1d(hidden, affine=False, eps=1e-6).train()
    ref_loss = F.cross_entropy(F.linear(bn(tok[:, 0]), ph["linear.weight"], ph["linear.bias"]), tg)
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < tol * abs(float(ref_loss.detach()))
    scale = float(pv["patch_embedding.position_embeddings"].grad.norm())
    errs = {}
    for k in trainable:
        got, ref = named[k].grad.float().cpu(), pv[k].grad
        if k == "norm.weight":
            assert float((got - ref).norm()) < tol * max(scale, float(ref.norm())), k
        elif k.endswith("qkv.bias"):
            assert (got - ref).abs().max() < 1e-6 + tol * ref.abs().max(), k
        else:
            errs[k] = rel_err(got, ref)
    print("per-parameter relative errors", {k: round(e, 5) for k, e in errs.items()})
    assert max(errs.values()) < tol, max(errs.items(), key=lambda kv: kv[1])
    assert (not lora) or sum("lora" in k for k in errs) == 8
    for k, v in cls.named_parameters():
        assert rel_err(v.grad, ph[k].grad) < tol, k
    g0 = vit._flat_grad.clone()
    vit.zero_grad()
    cls.zero_grad()
    cross_entropy(cls(vit(x.to(cuda))[0]), tg.to(cuda)).backward()
    assert torch.equal(g0, vit._flat_grad)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fresh_adapters_leave_rmsnorm_tokens_bit_equal(lib, cuda, dtype):
    from headct_foundation_amd import RMSNorm
    from headct_foundation_amd.dino_model import ViTBackbone
    torch.manual_seed(9)
    kw = dict(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, num_register_tokens=2,
              norm_layer=RMSNorm, compute_dtype=dtype)
    lora, plain = ViTBackbone(lora=True, **kw), ViTBackbone(lora=False, **kw)
    plain.load_state_dict({k: v for k, v in lora.state_dict().items() if "lora" not in k}, strict=True)
    lora, plain = lora.to(cuda), plain.to(cuda)
    x = (torch.rand(4, 3, 24, 24, 24) * 2.0).to(cuda)
    with torch.no_grad():
        want = plain(x)[0]
    tok = lora(x)[0]
    assert torch.equal(tok.detach(), want)
    R.case_loss(tok.float()).backward()
    for k, v in lora.named_parameters():
        if k.endswith("lora_matrix_A"):
            assert not v.grad.any(), k
        if k.endswith("lora_matrix_B"):
            assert v.grad.any() and torch.isfinite(v.grad).all(), k


# ---- 10. reproducibility and linearity in the batch ----------------------------------------------------------------------------
def test_step_is_bit_reproducible_and_linear_in_the_batch(lib, cuda):
    """`vitb_cut`, bf16, module default: a repeated step is bit-identical; the B = 8 step equals the mean of its two B = 4 halves
    (loss 2e-5, gradients 5e-3: the bars of tests/test_fullsize_gpu.py)."""
    cfg = O.CONFIGS["vitb_cut"]
    params = R.make_params(cfg, 3)
    x, noise = O.make_volume(cfg, 8, 3).to(cuda), O.make_noise(cfg, 8, 3).to(cuda)
    model = _build(cfg, params, cuda, "bf16", full_pred=False)
    loss1, g1 = _step(model, x, noise)
    loss2, g2 = _step(model, x, noise)
    assert loss1 == loss2 and all(torch.equal(g1[k], g2[k]) for k in g1), "the RMSNorm step is not bit-reproducible"
    half = _build(cfg, params, cuda, "bf16", full_pred=False)
    la, ga = _step(half, x[:4], noise[:4])
    lb, gb = _step(half, x[4:], noise[4:])
    assert abs(loss1 - 0.5 * (la + lb)) < 2e-5 * abs(loss1)
    worst = max((rel_err(g1[k], 0.5 * (ga[k] + gb[k])), k) for k in g1 if not k.endswith("qkv.bias"))
    assert worst[0] < 5e-3, worst


# ---- 11. the entry points ------------------------------------------------------------------------------------------------------
def test_main_pretrain_mae_rmsnorm_trains_saves_and_resumes(cuda, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(epochs, port, extra):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "main_pretrain_mae.py"), "--local_rank", "0", "--model_name", "mae",
               "--batch_size", "2", "--max_epochs", str(epochs), "--base_lr", "1.5e-4", "--cfg", os.path.join(ROOT, "configs/mae/mae_tiny_plumbing.yaml"),
               "--optimizer", "AdamW", "--scheduler", "cosine", "--weight_decay", "5e-3", "--grad_clip", "3.0"] + extra + [
               "--opts", "MAE.NORM_LAYER", "rmsnorm", "MODEL.DIR", str(tmp_path / "ckpt"), "LOG.OUTPUT_DIR", str(tmp_path / "log"),
               "OUTPUT", str(tmp_path / "json")]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return r.stdout + r.stderr
    log = run(2, 29541, [])
    assert "Train completed" in log and "Test completed" in log
    path = tmp_path / "ckpt" / "latest_mae_tiny.pt"
    ck = torch.load(path, map_location="cpu", weights_only=True)
    keys = [k[len("module."):] for k in ck["state_dict"]]
    assert "blocks.0.att_norm.weight" in keys and "decoder_norm.weight" in keys and not any(R.is_norm_bias(k) for k in keys)
    assert ck["epoch"] == 1 and float(ck["optimizer"]["state"][0]["step"]) == 8.0
    log = run(3, 29542, ["--model_load_path", str(path)])  # resumes from its own checkpoint: weights, optimizer state, epoch index
    assert "Load Pretrained Model" in log and "Loaded epoch: 1" in log and "Train completed" in log
    assert "unexpected_keys=[]" in log.replace(" ", "") or "<All keys matched successfully>" in log
    ck2 = torch.load(path, map_location="cpu", weights_only=True)
    assert ck2["epoch"] == 2 and float(ck2["optimizer"]["state"][0]["step"]) > 8.0  # the optimizer went on from the saved step
    assert not any(R.is_norm_bias(k) for k in ck2["state_dict"])


def test_main_downstream_rmsnorm_trains_saves_and_resumes(lib, cuda, tmp_path):
    from headct_foundation_amd import RMSNorm
    from headct_foundation_amd.classifier import LinearClassifier
    from headct_foundation_amd.dino_model import ViTBackbone
    kw = dict(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, norm_layer=RMSNorm)
    pre = ViTBackbone(**kw)
    sd = {"module." + k: v for k, v in pre.state_dict().items()}
    sd["module.decoder_embed.weight"] = torch.zeros(8, 48)  # a pre-training checkpoint also holds the decoder
    torch.save({"state_dict": sd, "epoch": 3}, tmp_path / "pre.pt")
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("MODEL:\n  NAME: vit\n")

    def run(load, port):
        opts = ["MAE.NORM_LAYER", "rmsnorm", "DATA.SYNTHETIC", "True", "DATA.SYNTHETIC_SAMPLES", "8", "VIT.INPUT_SIZE", "24", "VIT.PATCH_SIZE", "12",
                "VIT.HIDDEN_SIZE", "48", "VIT.MLP_DIM", "96", "VIT.NUM_LAYERS", "2", "VIT.NUM_HEADS", "3", "TRAIN.VAL_EVERY", "1",
                "MODEL.DIR", str(tmp_path / "out"), "MODEL.SAVE_NAME", "ft.pt", "LOG.OUTPUT_DIR", str(tmp_path / "log"), "PREDS_SAVE_NAME", "run"]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-port", str(port),
               os.path.join(ROOT, "main_downstream.py"), "--cfg", str(cfg), "--model_name", "vit", "--model_load_path", str(load),
               "--classifier", "linear", "--batch_size", "4", "--max_epochs", "2", "--grad_clip", "1.0", "--base_lr", "1e-4", "--opts"] + opts
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        log = r.stdout + r.stderr
        assert r.returncode == 0, log[-4000:]
        assert "MulticlassAccuracy" in log and "Final test loss" in log, log[-4000:]
    run(tmp_path / "pre.pt", 29615)
    b = torch.load(tmp_path / "out" / "ft.pt", map_location="cpu", weights_only=True)
    assert not any(R.is_norm_bias(k) for k in b["state_dict"])
    ViTBackbone(**kw).load_state_dict(b["state_dict"], strict=True)
    assert any(not torch.equal(v, pre.state_dict()[k]) for k, v in b["state_dict"].items())  # it trained
    LinearClassifier(48, 2).load_state_dict(torch.load(tmp_path / "out" / "ft_classifier.pt", map_location="cpu", weights_only=True)["state_dict"], strict=True)
    run(tmp_path / "out" / "ft.pt", 29616)  # and starts again from the checkpoint it wrote
