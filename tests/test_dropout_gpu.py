"""GPU: dropout on the HIP path against tests/dropout_ref.py -- the keep mask bit for bit, the streaming pass, attention with dropout
(fp32-math and bf16 MFMA kernels), and the models: pinned-seed parity in fp32 and bf16, determinism, inertness at rate 0 and in
eval mode, LoRA, and short engine-style runs."""
import dataclasses
import logging

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from headct_foundation_amd import _lib, dropout
from headct_foundation_amd._lib import HCT_BF16, HCT_F32
from oracle import mae_oracle as O
from tests import attention_ref as A
from tests import dropout_ref as R
from tests import lora_ref
from tests.util import grads_by_name, rel_err

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15  # a seed with both key words in use
P_MODEL = 0.25


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dt(t):
    return HCT_BF16 if t.dtype == torch.bfloat16 else HCT_F32


def _rand(shape, dev, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(dev)


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
# [3, 20]: the last group is a tail; [34, 768]; 1 100 003 elements: more groups than one sweep of the grid (1024 blocks x 256 threads
# x 4 elements), so threads loop, and a ragged tail
@pytest.mark.parametrize("shape", [(3, 20), (34, 768), (1100003,), (2, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_streaming_mask_is_the_numpy_mask(lib, cuda, shape, p):
    got = dropout.keep_mask(SEED, 7, shape, p, device=cuda).cpu().numpy()
    assert np.array_equal(got, R.stream_mask(SEED, 7, shape, p))
    assert not np.array_equal(got, R.stream_mask(SEED, 8, shape, p)) or got.size < 16


# 217: the MAE decoder; 289 and 513: the lengths of the 16-wave backward (one key in the last 32-key step); (3, 3, 65): nine (batch, head)
# items, so that the item index -- a counter word -- is above 8
@pytest.mark.parametrize("B,H,N", [(2, 3, 17), (2, 2, 65), (1, 2, 145), (1, 2, 217), (1, 2, 289), (1, 1, 513), (3, 3, 65)])
def test_attention_mask_is_the_numpy_mask(lib, cuda, B, H, N):
    for p in (0.1, 0.5):
        got = dropout.keep_mask(SEED, 5, (B, H, N, N), p, attention=True, device=cuda).cpu().numpy()
        assert np.array_equal(got, R.attn_mask(SEED, 5, B, H, N, p))


# ---- the streaming pass --------------------------------------------------------------------------------------------------------------
def _apply(lib, x, y, res, x2, y2, batches, stride, off, seg, site, p):
    _lib.check(lib.hct_dropout_apply(x.data_ptr(), _dt(x), y.data_ptr(), _dt(y), _lib.ptr(res), _lib.ptr(x2), _lib.ptr(y2), batches, stride, off,
                                     seg, SEED, site, p, _st()), "hct_dropout_apply")
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("second", [False, True])
def test_streaming_apply(lib, cuda, dtype, residual, second):
    p, site, shape = 0.25, 11, (37, 100)  # 3700 elements
    x, x2 = _rand(shape, cuda, dtype, 1), _rand(shape, cuda, dtype, 2)
    res = _rand(shape, cuda, torch.float32, 3) if residual else None
    out_dtype = torch.float32 if residual else dtype
    y = torch.full(shape, float("nan"), dtype=out_dtype, device=cuda)
    y2 = torch.full(shape, float("nan"), dtype=out_dtype, device=cuda) if second else None
    _apply(lib, x, y, res, x2 if second else None, y2, 1, 0, 0, x.numel(), site, p)
    Z = torch.from_numpy(R.stream_mask(SEED, site, shape, p)).to(cuda).float() * R.scale(p)
    want = x.float() * Z + (res if residual else 0)
    if out_dtype == torch.float32:
        assert torch.equal(y, want)
    else:  # one rounding of the exact fp32 value
        assert torch.equal(y, want.to(dtype))
    if second:
        assert torch.equal(y2, (x2.float() * Z).to(out_dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_streaming_apply_on_a_row_range_in_place(lib, cuda, dtype):
    """Rows 2 .. 4 of [2, 5, 64], in place: the other rows stay, the mask is that of the element's index in the whole tensor."""
    p, site, shape = 0.5, 0, (2, 5, 64)
    x = _rand(shape, cuda, dtype, 4)
    before = x.clone()
    _apply(lib, x, x, None, None, None, 2, 5 * 64, 2 * 64, 3 * 64, site, p)
    Z = torch.from_numpy(R.stream_mask(SEED, site, shape, p)).to(cuda).float() * R.scale(p)
    assert torch.equal(x[:, :2], before[:, :2])
    assert torch.equal(x[:, 2:], (before.float() * Z).to(dtype)[:, 2:])
    # a ragged whole tensor: the last group has three elements
    v = _rand((11,), cuda, dtype, 5)
    out = torch.empty_like(v)
    _apply(lib, v, out, None, None, None, 1, 0, 0, 11, site, p)
    assert torch.equal(out, (v.float() * torch.from_numpy(R.stream_mask(SEED, site, (11,), p)).to(cuda).float() * R.scale(p)).to(dtype))


# ---- attention with dropout ----------------------------------------------------------------------------------------------------------
def _attn_run(lib, qkv, d_o, B, N, H, dh, p, site, plain=False):
    dt = _dt(qkv)
    o = torch.full((B, N, H * dh), float("nan"), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, N, dtype=torch.float32, device=qkv.device)
    dqkv = torch.full_like(qkv, float("nan"))
    if plain:
        _lib.check(lib.hct_attention_fwd(qkv.data_ptr(), B, N, H, dh, dt, o.data_ptr(), lse.data_ptr(), _st()), "fwd")
        _lib.check(lib.hct_attention_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), B, N, H, dh, dt, dqkv.data_ptr(), _st()), "bwd")
    else:
        _lib.check(lib.hct_attention_dropout_fwd(qkv.data_ptr(), B, N, H, dh, dt, p, SEED, site, o.data_ptr(), lse.data_ptr(), _st()), "dropout fwd")
        _lib.check(lib.hct_attention_dropout_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), B, N, H, dh, dt, p, SEED, site,
                                                 dqkv.data_ptr(), _st()), "dropout bwd")
    torch.cuda.synchronize()
    return o, lse, dqkv


def _attn_ref(qkv, d_o, B, N, H, dh, p, site):
    """fp64 restatement on the storage values, with the numpy mask."""
    qr = qkv.double().requires_grad_(True)
    q, k, v = qr.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    Z = torch.from_numpy(R.attn_mask(SEED, site, B, H, N, p)).to(qkv.device).double() * R.scale(p)
    o = R.sdpa_dropout(q, k, v, Z).transpose(1, 2).reshape(B, N, H * dh)
    (o * d_o.double()).sum().backward()
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    return o.detach(), torch.logsumexp(s, -1).detach(), qr.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32math", "bf16mfma"])
@pytest.mark.parametrize("dh", [48, 64])
@pytest.mark.parametrize("N", [17, 65, 145])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_dropout_fwd_bwd(lib, cuda, dtype, dh, N, p):
    B, H, site = 2, 2, 9
    qkv = _rand((B, N, 3 * H * dh), cuda, dtype, 21)
    d_o = _rand((B, N, H * dh), cuda, dtype, 22)
    o_ref, lse_ref, dq_ref = _attn_ref(qkv, d_o, B, N, H, dh, p, site)
    o, lse, dqkv = _attn_run(lib, qkv, d_o, B, N, H, dh, p, site)
    e_o, e_d = rel_err(o, o_ref), rel_err(dqkv, dq_ref)
    print(f"attention dropout {dtype} dh {dh} N {N} p {p}: o {e_o:.2e} dqkv {e_d:.2e} lse {float((lse - lse_ref).abs().max()):.2e}")
    tol = 1e-3 if dtype == torch.float32 else 2e-2
    assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o.float()).all()
    assert e_o <= tol and e_d <= tol
    assert (lse - lse_ref).abs().max() < (1e-4 if dtype == torch.float32 else 2e-2)  # the normaliser is that of the undropped row
    # per part: a wrong mask in one of the three gradients cannot hide behind the other two
    g, gr = dqkv.view(B, N, 3, H * dh).float(), dq_ref.view(B, N, 3, H * dh)
    for i in range(3):
        assert rel_err(g[:, :, i], gr[:, :, i]) <= tol, "qkv"[i]


# Every instance attention_dropout_fwd_mfma / attention_dropout_bwd_mfma can launch (attn_fwd_mfma_kernel<dh, true>, attn_bwd2_mfma_kernel<dh,
# NW, true>), at both head dims, on either side of the 64 KiB of LDS above which the launch goes through hipFuncSetAttribute (forward 256
# Npad bytes, backward 264 Npad):
#   64   NW = 4, no padded key at all                      256  a multiple of 32; the first backward above 64 KiB (67 584 B)
#   217  the MAE decoder; NW = 8; 9 real keys in the tail   288  the last NW = 8 (76 032 B); the first forward above 64 KiB (73 728 B)
#   289  the first NW = 16; a 32-key step with one real key 513  the ViT-L decoder        608  the longest attention_mfma_supported accepts
#   609  (head dim 48) bf16 storage on the fp32-math kernels
#   65 with B = H = 3: nine workgroups, so xcd_bh() takes both of its branches (its value is also a Philox counter word)
_EVERY = [c + (torch.bfloat16,) for c in A.EVERY_INSTANCE] + [(1, 2, N, dh, torch.float32) for N in (217, 289) for dh in (48, 64)]
assert A.SEED == SEED


@pytest.mark.parametrize("inputs", ["gaussian", "flat"])
@pytest.mark.parametrize("B,H,N,dh,dtype", _EVERY, ids=lambda v: str(v).replace("torch.", ""))
def test_attention_dropout_every_instance(lib, cuda, B, H, N, dh, dtype, inputs):
    """gaussian: the assertions of test_attention_dropout_fwd_bwd.  flat (q x 0.05, every key carries about 1 / N of a row): besides
    those, every single row of o and of dV against the fp64 reference, under 3 x the error that the roundings no bf16 kernel avoids
    leave in the worst row of this very case (attention_ref.rounded) -- a bar that tests/test_attention_ref_cpu.py shows to be at most
    half of what ONE wrong keep decision moves a row by.  fp32 storage: the file's fp32 bars alone."""
    bf = dtype == torch.bfloat16
    tol, lse_tol = (2e-2, 2e-2) if bf else (1e-3, 1e-4)
    for p in ((0.1, 0.5) if inputs == "gaussian" or not bf else A.flat_rates(N)):
        case = A.row_case(B, H, N, dh, p) if inputs == "flat" and bf else None
        if case is not None:
            qkv, d_o, o_ref, lse_ref, dq_ref = case.qkv, case.d_o, case.o, case.lse, case.dqkv
        else:
            qkv, d_o = A.make_inputs(inputs, B, N, H, dh, dtype, seed=21 if inputs == "gaussian" else 31)
            o_ref, lse_ref, dq_ref = A.exact(qkv, d_o, B, N, H, dh, A.keep_multiplier(B, H, N, p, SEED, A.SITE))
        o, lse, dqkv = _attn_run(lib, qkv.to(cuda), d_o.to(cuda), B, N, H, dh, p, A.SITE)
        o, lse, dqkv = o.cpu(), lse.cpu(), dqkv.cpu()
        e_o, e_d, e_l = rel_err(o, o_ref), rel_err(dqkv, dq_ref), float((lse - lse_ref).abs().max())
        print(f"every instance {inputs} {dtype} B {B} H {H} N {N} dh {dh} p {p}: o {e_o:.2e} dqkv {e_d:.2e} (bar {tol:.0e}) lse {e_l:.2e} (bar {lse_tol:.0e})")
        if case is not None:
            r_o, r_v = A.row_err(o, o_ref, dh), A.row_err(A.parts(dqkv, B, N, H, dh)[2], case.dv, dh)
            print(f"    worst row: o {r_o:.2e} (bar {case.bar['o']:.2e}, one flip >= {case.flip['o']:.2e})  "
                  f"dV {r_v:.2e} (bar {case.bar['dv']:.2e}, one flip >= {case.flip['dv']:.2e})")
        assert torch.isfinite(dqkv.float()).all() and torch.isfinite(o.float()).all()
        assert e_o <= tol and e_d <= tol
        assert e_l < lse_tol  # the normaliser is that of the undropped row
        g, gr = dqkv.view(B, N, 3, H * dh).float(), dq_ref.view(B, N, 3, H * dh)
        for i in range(3):
            assert rel_err(g[:, :, i], gr[:, :, i]) <= tol, "qkv"[i]
        if case is not None:
            assert case.bar["o"] <= case.flip["o"] / 2 and case.bar["dv"] <= case.flip["dv"] / 2
            assert r_o <= case.bar["o"], (r_o, case.bar["o"])
            assert r_v <= case.bar["dv"], (r_v, case.bar["dv"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32math", "bf16mfma"])
@pytest.mark.parametrize("dh,N", [(48, 65), (64, 145), (48, 289), (64, 513)])
def test_attention_dropout_at_rate_zero_is_the_plain_attention(lib, cuda, dtype, dh, N):
    B, H = 2, 2
    qkv = _rand((B, N, 3 * H * dh), cuda, dtype, 23)
    d_o = _rand((B, N, H * dh), cuda, dtype, 24)
    o0, lse0, dq0 = _attn_run(lib, qkv, d_o, B, N, H, dh, 0.0, 0, plain=True)
    o, lse, dq = _attn_run(lib, qkv, d_o, B, N, H, dh, 0.0, 3)
    tol = 1e-3 if dtype == torch.float32 else 2e-2
    assert rel_err(o, o0) <= tol and rel_err(dq, dq0) <= tol and (lse - lse0).abs().max() < (1e-4 if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("dh,N", [(48, 65), (64, 145)])
def test_mfma_and_fp32_math_kernels_draw_the_same_mask(lib, cuda, dh, N):
    B, H, p, site = 2, 2, 0.5, 4
    qkv = _rand((B, N, 3 * H * dh), cuda, torch.bfloat16, 25)
    d_o = _rand((B, N, H * dh), cuda, torch.bfloat16, 26)
    o, _, dq = _attn_run(lib, qkv, d_o, B, N, H, dh, p, site)
    lib.hct_debug_force_simple_attention(1)
    try:
        o1, _, dq1 = _attn_run(lib, qkv, d_o, B, N, H, dh, p, site)
    finally:
        lib.hct_debug_force_simple_attention(0)
    # one different keep decision in a row of 65 at p = 0.5 moves that output row by ~1 / sqrt(65) of its norm: far above the bf16 bar
    assert rel_err(o, o1) <= 2e-2 and rel_err(dq, dq1) <= 2e-2


# ---- models --------------------------------------------------------------------------------------------------------------------------
def _mae(cfg, params, cuda, dtype, rate):
    from headct_foundation_amd import MaskedAutoencoderViT
    m = MaskedAutoencoderViT(**dict(cfg.ctor_kwargs(), dropout_rate=rate), compute_dtype=dtype)
    m.load_state_dict(params, strict=True)
    return m.to(cuda)


def _mae_step(m, x, noise, seed=None):
    m.zero_grad()
    if seed is not None:
        m.set_dropout_seed(seed)
    loss, _, _ = m(x, noise=noise)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), grads_by_name(m)


def _mae_case(name, use_bias):
    cfg = O.CONFIGS[name]
    if use_bias is not None:
        cfg = dataclasses.replace(cfg, use_bias=use_bias)
    return cfg, O.make_params(cfg, 0), O.make_volume(cfg, 2, 0), O.make_noise(cfg, 2, 0)


@pytest.mark.parametrize("name,use_bias", [("micro", True), ("micro", False), ("tiny", None)])
def test_mae_fp32_pinned_seed_vs_restatement(lib, cuda, name, use_bias):
    cfg, params, x, noise = _mae_case(name, use_bias)
    m = _mae(cfg, params, cuda, "fp32", P_MODEL).train()
    loss, grads = _mae_step(m, x.to(cuda), noise.to(cuda), SEED)
    assert m.last_dropout_seed == SEED
    r_loss, r_grads = R.mae_forward_backward(cfg, params, x, noise, R.Masks(SEED, P_MODEL))
    # the comparison discriminates: without the masks the restated gradients are elsewhere by a hundred times the bar
    o_grads = O.forward_backward(cfg, params, x, noise)[3]
    assert min(rel_err(o_grads[k], r_grads[k]) for k in r_grads if k.endswith("linear1.weight")) > 0.1
    assert abs(loss - float(r_loss)) <= 1e-3 * abs(float(r_loss))
    assert set(grads) == set(r_grads)
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print("worst gradient", name, use_bias, worst)
    assert worst[0] <= 1e-3, worst
    for k in grads:  # the bias gradients of proj / linear2 take the column sums of the masked gradient
        if k.endswith(("proj.bias", "linear2.bias")):
            assert (grads[k] - r_grads[k]).abs().max() <= 1e-6 + 1e-3 * r_grads[k].abs().max(), k


def test_mae_bf16_vs_bf16_storage_restatement(lib, cuda):
    """The bars of test_bf16_gradients_vs_bf16_storage_oracle (loss 1e-3, per-tensor gradient 2e-2, qkv.bias aside) with the same masks."""
    cfg, params, x, noise = _mae_case("tiny", None)
    m = _mae(cfg, params, cuda, "bf16", P_MODEL).train()
    loss, grads = _mae_step(m, x.to(cuda), noise.to(cuda), SEED)
    old = O._EMU[0]
    O._EMU[0] = True
    try:
        r_loss, r_grads = R.mae_forward_backward(cfg, params, x, noise, R.Masks(SEED, P_MODEL))
    finally:
        O._EMU[0] = old
    bad = sorted((rel_err(grads[k], r_grads[k]), k) for k in grads if not k.endswith("qkv.bias"))
    print("bf16 loss", loss, float(r_loss), "worst gradients", bad[-3:])
    assert abs(loss - float(r_loss)) <= 1e-3 * abs(float(r_loss))
    assert bad[-1][0] <= 2e-2, bad[-5:]


def _vit(dtype, rate, lora=False, cuda=None):
    from headct_foundation_amd.dino_model import ViTBackbone
    c = R.VIT_CASE
    m = ViTBackbone(**{k: c[k] for k in ("in_chans", "img_size", "patch_size", "hidden_size", "mlp_dim", "num_layers", "num_heads",
                                       "num_register_tokens", "qkv_bias")}, lora=lora, dropout_rate=rate, compute_dtype=dtype)
    p = O.make_vit_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, c["seed"])
    for k in p:  # adapters that do something, tokens that matter
        if k.endswith("lora_matrix_A"):
            p[k] = p[k] * 50.0
        if k.endswith("lora_matrix_B"):
            p[k] = p[k] * 0.25
        if k in ("cls_token", "register_tokens"):
            p[k] = p[k] * 5.0
    m.load_state_dict(p, strict=True)
    return m.to(cuda), p


def _vit_step(m, x, seed=None):
    m.zero_grad()
    if seed is not None:
        m.set_dropout_seed(seed)
    tok = m(x)[0]
    lora_ref.case_loss(tok).backward()
    torch.cuda.synchronize()
    return tok.detach().float().cpu(), grads_by_name(m)


def _vit_ref(p, x, masks, trainable=None):
    c = R.VIT_CASE
    pv = {k: v.clone().requires_grad_(trainable is None or trainable(k)) for k, v in p.items()}
    tok = R.vit_forward(pv, x, c["patch_size"], c["num_heads"], c["num_layers"], masks)
    lora_ref.case_loss(tok).backward()
    return tok.detach(), {k: v.grad for k, v in pv.items() if v.grad is not None}


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_vit_backbone_pinned_seed_vs_restatement(lib, cuda, dtype, tol):
    """fp32: 1e-3; bf16: the bar of the LoRA full-step test against the fp32 restatement (5e-2), same masks."""
    m, p = _vit(dtype, P_MODEL, cuda=cuda)
    x = R.vit_case_input()
    tok, grads = _vit_step(m.train(), x.to(cuda), SEED)
    r_tok, r_grads = _vit_ref(p, x, R.Masks(SEED, P_MODEL))
    plain, _ = _vit_ref(p, x, R.Ones())
    assert rel_err(r_tok, plain) > 0.05, "dropout at 0.25 moves the tokens"
    assert rel_err(tok, r_tok) <= tol
    assert set(grads) == set(r_grads)
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    print("worst gradient", dtype, worst)
    assert worst[0] <= tol, worst


def test_vit_lora_step_vs_restatement(lib, cuda):
    from headct_foundation_amd.misc import set_requires_grad_false
    m, p = _vit("fp32", P_MODEL, lora=True, cuda=cuda)
    set_requires_grad_false(m, lora=True)
    x = R.vit_case_input()
    tok, grads = _vit_step(m.train(), x.to(cuda), SEED)
    r_tok, r_grads = _vit_ref(p, x, R.Masks(SEED, P_MODEL), trainable=lora_ref.trainable)
    assert rel_err(tok, r_tok) <= 1e-3
    assert set(grads) == set(r_grads) and sum("lora" in k for k in grads) == 8
    worst = max((rel_err(grads[k], r_grads[k]), k) for k in grads)
    assert worst[0] <= 1e-3, worst


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_determinism_and_seed_draw(lib, cuda, dtype):
    cfg, params, x, noise = _mae_case("micro", None)
    m = _mae(cfg, params, cuda, dtype, P_MODEL).train()
    xc, nc = x.to(cuda), noise.to(cuda)
    a = _mae_step(m, xc, nc, 1234)
    b = _mae_step(m, xc, nc, 1234)
    c = _mae_step(m, xc, nc, 1235)
    assert a[0] == b[0] and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert a[0] != c[0]
    # unpinned: the seed comes from torch's CPU generator -- reproducible under manual_seed, fresh per forward
    torch.manual_seed(77)
    d = _mae_step(m, xc, nc)
    s1 = m.last_dropout_seed
    e = _mae_step(m, xc, nc)
    s2 = m.last_dropout_seed
    torch.manual_seed(77)
    f = _mae_step(m, xc, nc)
    assert s1 != s2 and m.last_dropout_seed == s1 and d[0] == f[0] and d[0] != e[0]
    # a model at rate 0 draws nothing
    m0 = _mae(cfg, params, cuda, dtype, 0.0).train()
    torch.manual_seed(5)
    want = torch.rand(3)
    torch.manual_seed(5)
    _mae_step(m0, xc, nc)
    assert torch.equal(torch.rand(3), want) and m0.last_dropout_seed is None


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eval_mode_and_rate_zero_are_inert(lib, cuda, dtype):
    cfg, params, x, noise = _mae_case("micro", None)
    xc, nc = x.to(cuda), noise.to(cuda)
    m0 = _mae(cfg, params, cuda, dtype, 0.0).train()
    md = _mae(cfg, params, cuda, dtype, P_MODEL)
    # eval mode at rate 0.25 == rate 0, forward and backward, bit for bit
    want = _mae_step(m0, xc, nc)
    got = _mae_step(md.eval(), xc, nc)
    assert want[0] == got[0] and all(torch.equal(want[1][k], got[1][k]) for k in want[1])
    assert md.last_dropout_seed is None
    with torch.no_grad():
        assert float(md(xc, noise=nc)[0]) == float(m0.eval()(xc, noise=nc)[0])
    # ... and after a dropped step the same model in eval mode is still the rate-0 model
    _mae_step(md.train(), xc, nc, 3)
    got = _mae_step(md.eval(), xc, nc)
    want = _mae_step(m0.train(), xc, nc)
    assert want[0] == got[0] and all(torch.equal(want[1][k], got[1][k]) for k in want[1])
    # the ViT backbone likewise
    v0, _ = _vit(dtype, 0.0, cuda=cuda)
    vd, _ = _vit(dtype, P_MODEL, cuda=cuda)
    xv = R.vit_case_input().to(cuda)
    a, b = _vit_step(v0.train(), xv), _vit_step(vd.eval(), xv)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


def test_rate_zero_training_step_is_what_the_oracle_pins(lib, cuda):
    """A dropout_rate = 0 model in training mode: the step tests/test_model_gpu.py holds against the oracle (fp32, 1e-3)."""
    cfg, params, x, noise = _mae_case("micro", None)
    loss, grads = _mae_step(_mae(cfg, params, cuda, "fp32", 0.0).train(), x.to(cuda), noise.to(cuda))
    o_loss, _, _, o_grads, _ = O.forward_backward(cfg, params, x, noise)
    assert abs(loss - float(o_loss)) <= 1e-3 * abs(float(o_loss))
    assert max(rel_err(grads[k], o_grads[k]) for k in grads) <= 1e-3


# ---- engine-style runs ---------------------------------------------------------------------------------------------------------------
def test_mae_engine_run_with_dropout(lib, cuda):
    """Three iterations of engine_pretrain_mae.train_one_epoch at MAE.DROPOUT_RATE 0.1, then its validation pass: finite losses of the
    same order, and the validation loss of the dropout model is that of a rate-0 model holding the same weights."""
    import engine_pretrain_mae as E
    from headct_foundation_amd.cfgnode import CfgNode
    from headct_foundation_amd.lr_sched import get_cosine_schedule_with_warmup
    from headct_foundation_amd.optim import HipAdamW
    cfg, params, _, _ = _mae_case("micro", None)
    ecfg = CfgNode()
    ecfg.MODEL = CfgNode(); ecfg.MODEL.NAME = "mae"
    ecfg.TRAIN = CfgNode(); ecfg.TRAIN.GRAD_CLIP = 3.0
    log = logging.getLogger("dropout_engine")
    log.propagate = False
    m = _mae(cfg, params, cuda, "bf16", 0.1)
    opt = HipAdamW(m, lr=1e-3, weight_decay=5e-3, betas=(0.9, 0.95))
    sch = get_cosine_schedule_with_warmup(opt, 1, 10, lr_end=1e-6)
    batches = [O.make_volume(cfg, 2, 40 + i) for i in range(3)]
    torch.manual_seed(1)
    stats = E.train_one_epoch(ecfg, m, batches, opt, sch, 0, 1, logger=log, device=cuda)
    first = float(O.forward_backward(cfg, params, batches[0], O.make_noise(cfg, 2, 0))[0])
    assert np.isfinite(stats["loss"]) and 0.2 * first < stats["loss"] < 5 * first and m.last_dropout_seed is not None
    m0 = _mae(cfg, {k: v.detach().cpu() for k, v in m.state_dict().items()}, cuda, "bf16", 0.0)
    vals = []
    for model in (m, m0):
        torch.manual_seed(2)  # the validation masks
        vals.append(E.val_one_epoch(ecfg, model, batches, 0, 1, logger=log, device=cuda)["loss"])
    assert vals[0] == vals[1] and np.isfinite(vals[0])


def test_downstream_style_run_with_dropout(lib, cuda):
    """Three fine-tuning steps (linear classifier, synthetic labelled volumes, cut ViT) at VIT.DROPOUT_RATE 0.1, then an evaluation pass
    that equals the rate-0 backbone's on the same weights."""
    from headct_foundation_amd import LinearClassifier, cross_entropy
    from headct_foundation_amd.data import SyntheticLabelled
    from headct_foundation_amd.dino_model import ViTBackbone
    from headct_foundation_amd.optim import HipAdamW, clip_grad_norm_
    torch.manual_seed(5)
    kw = dict(in_chans=3, img_size=24, patch_size=12, hidden_size=48, mlp_dim=96, num_layers=2, num_heads=3, compute_dtype="bf16")
    vit = ViTBackbone(**kw, dropout_rate=0.1).to(cuda)
    cls = LinearClassifier(48, 2, feature_grad=True).to(cuda).train()
    opts = [HipAdamW(cls, lr=1e-3, weight_decay=0.04), HipAdamW(vit, lr=1e-4, weight_decay=0.04)]
    v, t, _ = SyntheticLabelled(1, 8, 3, 24, 2, cuda, seed=0).batches[0]
    losses = []
    vit.train()
    for _ in range(3):
        for o in opts:
            o.zero_grad()
        loss = cross_entropy(cls(vit(v)[0]), t)
        loss.backward()
        clip_grad_norm_(cls, 1.0)
        clip_grad_norm_(vit, 1.0)
        for o in opts:
            o.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)) and max(losses) < 5 * min(losses) and vit.last_dropout_seed is not None
    v0 = ViTBackbone(**kw)
    v0.load_state_dict({k: p.detach().cpu() for k, p in vit.state_dict().items()}, strict=True)
    v0 = v0.to(cuda).eval()
    cls.eval()
    with torch.no_grad():
        a, b = cls(vit.eval()(v)[0]), cls(v0(v)[0])
    assert torch.equal(a, b) and float(F.cross_entropy(a.float(), t.long())) == float(F.cross_entropy(b.float(), t.long()))
